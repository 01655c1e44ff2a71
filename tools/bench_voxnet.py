"""Time one train step of the VoxNet classifier (papc_amd.models.VoxNet), on the voxconv kernels and on the torch-op path.

    python tools/bench_voxnet.py [--batches 64,1] [--steps 50] [--warmup 10] [--repeats 5] [--kernels]

Step = forward + softmax cross-entropy (head.softmax_cross_entropy) + backward + Adam on the flat parameter buffer
(papc_amd.distributed.FlatAdam), timed eagerly and as a captured hipGraph replay, for each batch size with the kernels
(csrc/voxconv.hip) and with the backbone in torch device ops (what PAPC_VOXNET=0 selects: im2col copies + matmul, the baseline), in one
process on the same occupancy grids (1024 random points per cloud).  Every figure is the median of ``repeats`` timings of ``steps`` steps;
min and max are the run-to-run spread.  ``launches`` counts the device kernels of one eager step (torch profiler).  ``--kernels`` adds the
per-kernel device times of one profiled eager step of the kernel path at the first batch size (the two Linear layers' launches among
them).  Prints one JSON line.
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
    ap.add_argument("--batches", default="64,1")
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    from torch.profiler import ProfilerActivity, profile
    from papc_amd import head as H
    from papc_amd import voxnet
    from papc_amd.distributed import FlatAdam, FlatParams
    from papc_amd.models import VoxNet

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

    def kernel_times(prof):
        rows = [(e.key.split("(")[0], e.count, e.device_time_total) for e in prof.key_averages()
                if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.key and "Memset" not in e.key]
        rows.sort(key=lambda r: -r[2])
        return [{"kernel": k[-60:], "launches": int(c), "us": round(t, 1)} for k, c, t in rows]

    results, per_kernel = [], None
    for B in [int(v) for v in a.batches.split(",")]:
        rng = np.random.default_rng(0)
        x = voxnet.occupancy_grid(torch.from_numpy(rng.uniform(-1.0, 1.0, size=(B, 1024, 3)).astype(np.float32)).to(dev))
        y = torch.from_numpy(rng.integers(0, a.classes, size=B)).to(dev)
        for path in ("kernel", "torch ops"):
            voxnet._VOXNET = path == "kernel"
            torch.manual_seed(0)
            model = VoxNet(num_classes=a.classes).to(dev).train()
            flat = FlatParams(model)
            opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)

            def step():
                loss = H.softmax_cross_entropy(model(x), y)
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
            launches = int(sum(e.count for e in prof.key_averages()
                               if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.key and "Memset" not in e.key))      # device kernels only
            if a.kernels and per_kernel is None and path == "kernel":
                per_kernel = {"batch": B, "kernels": kernel_times(prof)}
            eager = spread(step)
            g = torch.cuda.CUDAGraph()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    step()
            torch.cuda.current_stream().wait_stream(s)
            timed(g.replay, a.warmup)
            graph = spread(g.replay)
            results.append({"batch": B, "backbone": path, "launches_per_step": launches, "eager": eager, "graph": graph,
                            "graph_clouds_per_s": round(B * 1e3 / graph["ms_per_step"], 1)})
            del g
    out = {"model": "VoxNet", "edge": 32, "classes": a.classes, "steps": a.steps, "repeats": a.repeats, "results": results}
    if per_kernel is not None:
        out["profiled_step"] = per_kernel
    print(json.dumps(out))


if __name__ == "__main__":
    main()
