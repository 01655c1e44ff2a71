"""Time one train step of the PointPillars RPN (papc_amd.rpn.RPN) at the KITTI car shape, on the conv2d kernels and on the torch-op path.

    python tools/bench_rpn.py [--batches 1,2] [--steps 5] [--warmup 2] [--repeats 5] [--kernels] [--paths kernel,torch]

Step = forward + a sum-of-outputs loss + backward + Adam on the flat parameter buffer (papc_amd.distributed.FlatAdam), timed eagerly and as a
captured hipGraph replay, for each batch size with the kernels (csrc/conv2d.hip) and with the module in torch device ops (what PAPC_RPN=0
selects: im2col views + matmul, the baseline), in one process on the same canvas: 64 x 496 x 432, zero except 12000 random pillar pixels per
frame (params/configs/pointpillars_kitti_car_xy16.yaml: filters [64, 128, 256], layer_nums [3, 5, 5]).  Every figure is the median of
``repeats`` timings of ``steps`` steps; min and max are the run-to-run spread.  ``launches`` counts the device kernels of one eager step
(torch profiler).  ``--kernels`` adds the per-kernel device times of one profiled eager step of the kernel path at the first batch size.
Prints one JSON line.
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

KITTI = dict(use_norm=True, num_class=1, layer_nums=[3, 5, 5], layer_strides=[2, 2, 2], num_filters=[64, 128, 256], upsample_strides=[1, 2, 4],
             num_upsample_filters=[128, 128, 128], num_input_filters=64, num_anchor_per_loc=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--ny", type=int, default=496)
    ap.add_argument("--nx", type=int, default=432)
    ap.add_argument("--pillars", type=int, default=12000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--paths", default="kernel,torch")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    from torch.profiler import ProfilerActivity, profile
    from papc_amd import rpn
    from papc_amd.distributed import FlatAdam, FlatParams

    dev = torch.device("cuda:0")

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    def spread(fn):
        ts = [timed(fn, a.steps) for _ in range(a.repeats)]
        return {"ms_per_step": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}

    def kernel_times(prof):
        rows = [(e.key.split("(")[0], e.count, e.device_time_total) for e in prof.key_averages()
                if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.key and "Memset" not in e.key]
        rows.sort(key=lambda r: -r[2])
        return [{"kernel": k[-60:], "launches": int(c), "us": round(t, 1)} for k, c, t in rows]

    results, per_kernel = [], None
    for B in [int(v) for v in a.batches.split(",")]:
        rng = np.random.default_rng(0)
        canvas = np.zeros((B, 64, a.ny * a.nx), np.float32)
        for b in range(B):
            cells = rng.choice(a.ny * a.nx, size=min(a.pillars, a.ny * a.nx), replace=False)
            canvas[b][:, cells] = np.abs(rng.normal(size=(64, cells.size))).astype(np.float32)      # a PFN output: post-ReLU, non-negative
        x = torch.from_numpy(canvas.reshape(B, 64, a.ny, a.nx)).to(dev)
        for path in a.paths.split(","):
            rpn._RPN = path == "kernel"
            torch.manual_seed(0)
            model = rpn.RPN(**KITTI).to(dev).train()
            flat = FlatParams(model)
            opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)

            def step():
                out = model(x)
                sum(v.sum() for v in out.values()).backward()
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
            row = {"batch": B, "path": path, "launches_per_step": launches, "eager": spread(step)}
            if not a.no_graph:
                g = torch.cuda.CUDAGraph()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    with torch.cuda.graph(g, stream=s):
                        step()
                torch.cuda.current_stream().wait_stream(s)
                timed(g.replay, a.warmup)
                row["graph"] = spread(g.replay)
                row["graph_frames_per_s"] = round(B * 1e3 / row["graph"]["ms_per_step"], 2)
                del g
            results.append(row)
            del model, flat, opt
            torch.cuda.empty_cache()
    out = {"model": "RPN", "canvas": [64, a.ny, a.nx], "config": "pointpillars_kitti_car_xy16", "steps": a.steps, "repeats": a.repeats, "results": results}
    if per_kernel is not None:
        out["profiled_step"] = per_kernel
    print(json.dumps(out))


if __name__ == "__main__":
    main()
