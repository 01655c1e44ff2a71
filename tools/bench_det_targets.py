"""Time the PointPillars training-target stage (papc_amd.targets): anchors_mask + assign as the fused launch sequences against the torch-op
flavour (PAPC_DET_TARGETS=0).

    python tools/bench_det_targets.py [--batches 2,4] [--pillars 12000] [--gts 20] [--steps 50] [--warmup 10] [--repeats 5]

Shape: the KITTI car config -- feature map 248 x 216 with two anchors per cell (A = 107 136), pillar grid 496 x 432 of 0.16 m cells, about 12 000
occupied pillars and about 20 ground-truth cars per frame, padded to Gmax = 32.  Inputs are synthetic: pillars on random distinct cells of the nearest 300 of the 432
cell columns (about 70 % of the anchors end inside the mask), cars of the anchor's size (+- 10 %) at random places and headings.  Both flavours run in one process on the same inputs, each in its own timed loop.
Every step (mask, then assign on that mask) is timed with device events, eagerly and -- where capture succeeds -- as a replayed single-stream
hipGraph; a figure is the median of ``repeats`` timings of ``steps`` steps, min and max the run-to-run spread.  ``launches`` counts the device
kernels of one eager step (torch profiler), ``kernel_us`` the device time of each of the fused flavour's in that step.  The torch-op flavour synchronises with the host (boolean indexing, num_gt), so it cannot be
captured: the tool reports that instead of a graph figure.  ``bytes_per_frame`` is what the fused kernels read and write by their own
arithmetic.  Reads nothing outside the repository.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,4")
    ap.add_argument("--pillars", type=int, default=12000)
    ap.add_argument("--gts", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()

    import torch
    from torch.profiler import ProfilerActivity, profile
    from papc_amd import targets as T

    dev = torch.device("cuda:0")

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n          # microseconds per step

    def spread(fn):
        ts = [timed(fn, a.steps) for _ in range(a.repeats)]
        return {"us_per_step": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}

    H, W, nx, ny, Gmax = 248, 216, 432, 496, 32
    near = 300                                        # the pillars lie in the nearest 300 of the 432 cell columns: about 70 % of the anchors are inside
    gen = T.AnchorGeneratorStride(sizes=[1.6, 3.9, 1.56], anchor_strides=[0.32, 0.32, 0.0], anchor_offsets=[0.16, -39.52, -1.78],
                                  rotations=[0, math.pi / 2], match_threshold=0.6, unmatch_threshold=0.45)
    cache = T.TargetAssigner([gen]).anchor_cache((1, H, W), [0.16, 0.16, 4.0], [0.0, -39.68, -3.0, 69.12, 39.68, 1.0], (nx, ny, 1), device=dev)
    A = int(cache["anchors"].shape[0])

    results = []
    for B in [int(v) for v in a.batches.split(",")]:
        g = torch.Generator().manual_seed(0)
        coors, boxes = [], torch.zeros(B, Gmax, 7)
        num_gt = torch.randint(max(a.gts - 4, 0), min(a.gts + 5, Gmax + 1), (B,), generator=g, dtype=torch.int32)
        for b in range(B):
            cell = torch.randperm(near * ny, generator=g)[:a.pillars]
            coors.append(torch.stack([torch.full_like(cell, b), torch.zeros_like(cell), cell // near, cell % near], dim=1))
            u = torch.rand(Gmax, 7, generator=g)
            boxes[b] = torch.stack([2.0 + 65.0 * u[:, 0], -37.0 + 74.0 * u[:, 1], -1.9 + 0.3 * u[:, 2], 1.6 * (0.9 + 0.2 * u[:, 3]),
                                    3.9 * (0.9 + 0.2 * u[:, 4]), 1.56 * (0.9 + 0.2 * u[:, 5]), math.pi * (2.0 * u[:, 6] - 1.0)], dim=1)
        coors = torch.cat(coors).int().to(dev)
        boxes, classes, num_gt = boxes.to(dev), torch.ones(B, Gmax, dtype=torch.int32, device=dev), num_gt.to(dev)
        ws = (torch.empty(T.mask_workspace_bytes(B, A, ny, nx), dtype=torch.uint8, device=dev),
              torch.empty(T.assign_workspace_bytes(B, A, Gmax), dtype=torch.uint8, device=dev))
        mask, out = torch.empty(B, A, dtype=torch.uint8, device=dev), {}
        for flavour, fused in (("fused", True), ("torch ops", False)):
            def step():
                T.anchors_mask(coors, B, cache, 1, out=mask, workspace=ws[0] if fused else None, fused=fused)
                return T.assign(cache, boxes, classes, num_gt, mask, out=out, workspace=ws[1] if fused else None, fused=fused)

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
                               if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.key and "Memset" not in e.key))
            r = step()
            row = {"batch": B, "flavour": flavour, "launches_per_step": launches, "eager": spread(step),
                   "inside_fraction": round(float(mask.float().mean()), 3), "num_pos": r["num_pos"].tolist()}
            if fused:
                dev_us = lambda e: getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)        # noqa: E731
                row["kernel_us"] = {e.key.split("(")[0].split("::")[-1]: round(dev_us(e) / max(e.count, 1), 2) for e in prof.key_averages()
                                    if str(e.device_type).endswith("CUDA") and "Memcpy" not in e.key}
                try:
                    graph = torch.cuda.CUDAGraph()
                    s.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(s):
                        with torch.cuda.graph(graph, stream=s):
                            step()
                    torch.cuda.current_stream().wait_stream(s)
                    timed(graph.replay, a.warmup)
                    row["graph"] = spread(graph.replay)
                    del graph
                except Exception as e:      # noqa: BLE001 -- report it, as the figure's absence must be explained
                    row["graph"] = "capture failed: %s" % str(e).splitlines()[0][:160]
                    torch.cuda.synchronize()
            else:
                row["graph"] = "not captured: this flavour reads num_gt and the mask on the host"
            results.append(row)
    # per frame: the map is cleared, counted into, scanned twice (read + write each) and gathered from; per anchor the mask kernel reads 16 B of
    # cells and writes 1 B, each assign pass reads 1 B of mask and -- for an inside anchor -- 16 B of near-bbox, and the second writes
    # 4 + 28 + 4 + 4 + 4 B and reads two thresholds
    bytes_per_frame = ny * nx * 4 * 5 + a.pillars * 16 + A * (16 + 1 + 4 * 4) + A * (1 + 16) + A * (1 + 16 + 8 + 44)
    print(json.dumps({"op": "anchors_mask + assign", "anchors": A, "pillar_grid": [ny, nx], "pillars": a.pillars, "gmax": Gmax, "steps": a.steps,
                      "repeats": a.repeats, "bytes_per_frame": bytes_per_frame, "results": results}))


if __name__ == "__main__":
    main()
