"""Time one train step of the PointNet part segmenters (papc_amd.models.PointNet_Seg / PointNet_Basic_Seg).

    python tools/bench_pointnet_seg.py [--model pointnet|pointnet_basic] [--batch 32] [--points 1024] [--steps 50] [--warmup 10]

Step = forward + mean per-point softmax cross-entropy (head.softmax_cross_entropy on the [B*N, parts] logits) + backward + Adam on the flat
parameter buffer (papc_amd.distributed.FlatAdam), timed eagerly and as a captured hipGraph replay.  N is the model's max_point / max_points
(the source tiles by it).  PAPC_SEG_CONCAT=0 runs seg_net[0] on the materialised concat (the baseline).  Prints one JSON line.
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
    ap.add_argument("--model", choices=["pointnet", "pointnet_basic"], default="pointnet_basic")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--parts", type=int, default=50)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()

    import numpy as np
    import torch
    from papc_amd import head as H
    from papc_amd import segment
    from papc_amd.distributed import FlatAdam, FlatParams
    from papc_amd.models import PointNet_Basic_Seg, PointNet_Seg

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cls = PointNet_Seg if a.model == "pointnet" else PointNet_Basic_Seg
    model = cls(a.parts, a.points).to(dev).train()
    flat = FlatParams(model)
    opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.normal(size=(a.batch, 3, a.points)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, a.parts, size=a.batch * a.points)).to(dev)
    one = H.unit_gradient(dev)

    def step():
        logits = model(x)
        loss = H.softmax_cross_entropy(logits.view(-1, a.parts), y)
        loss.backward(one)
        opt.step_dev(1.0, zero_grad=True, self_tick=True)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(a.warmup):
            step()
    torch.cuda.current_stream().wait_stream(s)
    eager_ms = timed(step, a.steps)
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            step()
    torch.cuda.current_stream().wait_stream(s)
    timed(g.replay, a.warmup)
    graph_ms = timed(g.replay, a.steps)
    print(json.dumps({"model": cls.__name__, "seg_concat": "kernel" if segment._SEG_CONCAT else "materialised", "batch": a.batch,
                      "points": a.points, "parts": a.parts, "steps": a.steps,
                      "eager_ms_per_step": round(eager_ms, 4), "eager_clouds_per_s": round(a.batch * 1e3 / eager_ms, 1),
                      "graph_ms_per_step": round(graph_ms, 4), "graph_clouds_per_s": round(a.batch * 1e3 / graph_ms, 1)}))


if __name__ == "__main__":
    main()
