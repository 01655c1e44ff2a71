"""Time one train step of the VFE models (papc_amd.models.VFE_Clas / VFE_Seg).

    python tools/bench_vfe.py [--model clas|seg] [--batch 32] [--points 1024] [--steps 50] [--warmup 10] [--repeats 5]

Step = forward + mean softmax cross-entropy (head.softmax_cross_entropy; the segmenter's on the [B*N, parts] logits) + backward + Adam on the
flat parameter buffer (papc_amd.distributed.FlatAdam), timed eagerly and as a captured hipGraph replay: ``repeats`` windows of ``steps`` steps
each, the median window reported with the spread (min .. max).  N is the model's max_points (the source tiles by it).  PAPC_VFE_CONCAT=0 runs
the two concat layers on the materialised concat (the baseline).  Prints one JSON line that names the path.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["clas", "seg"], default="seg")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=0, help="default: 16 (clas) / 50 (seg)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()

    import numpy as np
    import torch
    from papc_amd import head as H
    from papc_amd import vfe
    from papc_amd.distributed import FlatAdam, FlatParams
    from papc_amd.models import VFE_Clas, VFE_Seg

    if not torch.cuda.is_available():
        raise SystemExit("bench_vfe.py needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    nc = a.classes or (16 if a.model == "clas" else 50)
    model = (VFE_Clas(nc, a.points) if a.model == "clas" else VFE_Seg(256, nc, a.points)).to(dev).train()
    flat = FlatParams(model)
    opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.normal(size=(a.batch, 3, a.points)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, nc, size=a.batch * (1 if a.model == "clas" else a.points))).to(dev)
    one = H.unit_gradient(dev)

    def step():
        logits = model(x)
        loss = H.softmax_cross_entropy(logits.view(-1, nc), y)
        loss.backward(one)
        opt.step_dev(1.0, zero_grad=True, self_tick=True)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def windows(fn):
        ms = sorted(timed(fn, a.steps) for _ in range(a.repeats))
        return ms[len(ms) // 2], ms[0], ms[-1]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(a.warmup):
            step()
    torch.cuda.current_stream().wait_stream(s)
    eager = windows(step)
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            step()
    torch.cuda.current_stream().wait_stream(s)
    timed(g.replay, a.warmup)
    graph = windows(g.replay)
    print(json.dumps({"model": type(model).__name__, "vfe_concat": "kernel" if vfe._VFE_CONCAT else "materialised", "batch": a.batch,
                      "points": a.points, "classes": nc, "steps": a.steps, "repeats": a.repeats,
                      "eager_ms_per_step": round(eager[0], 4), "eager_ms_min_max": [round(eager[1], 4), round(eager[2], 4)],
                      "eager_clouds_per_s": round(a.batch * 1e3 / eager[0], 1),
                      "graph_ms_per_step": round(graph[0], 4), "graph_ms_min_max": [round(graph[1], 4), round(graph[2], 4)],
                      "graph_clouds_per_s": round(a.batch * 1e3 / graph[0], 1)}))


if __name__ == "__main__":
    main()
