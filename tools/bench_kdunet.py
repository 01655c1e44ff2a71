"""Time one train step of the KDUNet part segmenter (papc_amd.models.KDUNet), on the kdbn kernels and on the torch-op path.

    python tools/bench_kdunet.py [--batches 32,1] [--steps 50] [--warmup 10] [--repeats 5] [--levels]

Step = forward + per-point softmax cross-entropy (head.softmax_cross_entropy over the B * 1024 rows) + backward + Adam on the flat parameter
buffer (papc_amd.distributed.FlatAdam), timed eagerly and as a captured hipGraph replay, for each batch size with the down levels on the
kernels (csrc/kdbn.hip) and as the source's op sequence in torch device ops (what PAPC_KDCONV=0 selects: the baseline), in one process on the
same inputs.  The up half runs on the same nodes either way.  Split dims are one vector per cloud.  Every figure is the median of ``repeats``
timings of ``steps`` steps; min and max are the run-to-run spread.  ``launches`` counts the device kernels of one eager step (torch profiler);
``down_kernels_us`` / ``all_kernels_us`` are that step's device time in the kb_* kernels and in all kernels, so the rest is the up half, the
loss and the optimizer.  ``--levels`` also times each down level's node alone (forward, and forward + backward, hip events, median of
``repeats`` x ``steps``) on both paths at the first batch size.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--classes", type=int, default=50)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--levels", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    from torch.profiler import ProfilerActivity, profile
    from papc_amd import head as H
    from papc_amd import kdnet
    from papc_amd.distributed import FlatAdam, FlatParams
    from papc_amd.models import KDUNet, _KDUNetDown

    dev = torch.device("cuda:0")
    one = H.unit_gradient(dev)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def spread(fn):
        ts = [timed(fn, a.steps) for _ in range(a.repeats)]
        return {"ms_per_step": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}

    batches = [int(v) for v in a.batches.split(",")]
    results = []
    for B in batches:
        rng = np.random.default_rng(0)
        x = torch.from_numpy(rng.normal(size=(B, 3, 1024)).astype(np.float32)).to(dev)
        split = kdnet.pack_split_dims([rng.integers(0, 3, size=(B, d)) for d in kdnet.DIMS], B, dev)
        y = torch.from_numpy(rng.integers(0, a.classes, size=B * 1024)).to(dev)
        for path in ("kernel", "torch ops"):
            kdnet._KDCONV = path == "kernel"
            torch.manual_seed(0)
            model = KDUNet(num_classes=a.classes).to(dev).train()
            flat = FlatParams(model)
            opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)

            def step():
                loss = H.softmax_cross_entropy(model([x, split]).view(-1, a.classes), y)
                loss.backward(one)
                opt.step_dev(1.0, zero_grad=True, self_tick=True)

            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(a.warmup):
                    step()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step()
                torch.cuda.synchronize()
            kernels = [e for e in prof.key_averages() if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.key and "Memset" not in e.key]
            launches = int(sum(e.count for e in kernels))                                           # device kernels only
            dev_us = lambda e: float(getattr(e, "self_device_time_total", getattr(e, "self_cuda_time_total", 0.0)))      # noqa: E731
            eager = spread(step)
            g = torch.cuda.CUDAGraph()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    step()
            torch.cuda.current_stream().wait_stream(s)
            timed(g.replay, a.warmup)
            graph = spread(g.replay)
            results.append({"batch": B, "kdconv": path, "launches_per_step": launches, "eager": eager, "graph": graph,
                            "graph_clouds_per_s": round(B * 1e3 / graph["ms_per_step"], 1),
                            "down_kernels_us": round(sum(dev_us(e) for e in kernels if "kb_" in e.key), 1),
                            "all_kernels_us": round(sum(dev_us(e) for e in kernels), 1)})
            del g

    levels = []
    if a.levels:
        B = batches[0]
        g = torch.Generator().manual_seed(0)
        for dim, cin, f in _KDUNetDown.LEVELS:
            conv, bn = torch.nn.Conv1d(cin, 3 * f, 1).to(dev), torch.nn.BatchNorm1d(3 * f).to(dev)
            rows = (torch.randn(B * dim, cin, generator=g).abs() if cin > 3 else torch.randn(B * dim, cin, generator=g)).to(dev).requires_grad_(True)
            sel = torch.randint(0, 3, (B, dim), generator=g).int().to(dev)
            gout = torch.randn(B * dim // 2, f, generator=g).to(dev)
            row = {"dim": dim, "cin": cin, "f": f, "batch": B}
            for path in ("kernel", "torch ops"):
                kdnet._KDCONV = path == "kernel"

                def fwd():
                    with torch.no_grad():
                        kdnet.kdconv_bn(rows, sel, conv, bn, B, dim, True)

                def both():
                    kdnet.kdconv_bn(rows, sel, conv, bn, B, dim, True).backward(gout)
                    rows.grad = conv.weight.grad = conv.bias.grad = bn.weight.grad = bn.bias.grad = None

                for fn in (fwd, both):
                    timed(fn, a.warmup)
                tf, tb = spread(fwd), spread(both)
                row[path] = {"fwd_us": round(tf["ms_per_step"] * 1e3, 1), "fwd_min_max_us": [round(tf["min"] * 1e3, 1), round(tf["max"] * 1e3, 1)],
                             "fwd_bwd_us": round(tb["ms_per_step"] * 1e3, 1), "fwd_bwd_min_max_us": [round(tb["min"] * 1e3, 1), round(tb["max"] * 1e3, 1)]}
            levels.append(row)
    out = {"model": "KDUNet", "points": 1024, "classes": a.classes, "steps": a.steps, "repeats": a.repeats, "results": results}
    if levels:
        out["levels"] = levels
    print(json.dumps(out))


if __name__ == "__main__":
    main()
