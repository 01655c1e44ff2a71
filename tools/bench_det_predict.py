"""Time PointPillars predict_tensors (papc_amd.detect): the fused launch sequence against the torch-op flavour (PAPC_DET_POST=0).

    python tools/bench_det_predict.py [--batches 1,4] [--anchors 107136] [--pre 1000] [--post 300] [--thresh 0.15] [--fractions 0.01,0.2]
                                      [--steps 50] [--warmup 10] [--repeats 5]

Shape: the KITTI car config, A = 248 x 216 x 2 anchors on a 0.32 m grid (two per cell, r = 0 and pi/2), one class column, direction classifier
and rotated NMS on.  Inputs are synthetic: encodings N(0, 0.15), cold logits near -4, and a drawn fraction of the anchors (about 1 % and about
20 %) with logits U(-1.5, 3), i.e. above the 0.15 threshold.  Both flavours run in one process on the same inputs.  Every step is timed with device
events, eagerly and -- where capture succeeds -- as a replayed single-stream hipGraph; a figure is the median of ``repeats`` timings of ``steps``
steps, min and max the run-to-run spread.  ``launches`` counts the device kernels of one eager step (torch profiler).  The torch-op flavour
synchronises with the host (boolean indexing, the NMS count), so it cannot be captured: the tool reports that instead of a graph figure.
Reads nothing outside the repository.  Prints one JSON line.
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
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--anchors", type=int, default=107136)
    ap.add_argument("--pre", type=int, default=1000)
    ap.add_argument("--post", type=int, default=300)
    ap.add_argument("--thresh", type=float, default=0.15)
    ap.add_argument("--fractions", default="0.01,0.2")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()

    import torch
    from torch.profiler import ProfilerActivity, profile
    from papc_amd import detect as D

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

    A = a.anchors
    W = 216
    cell = torch.arange(A // 2)
    anchors = torch.zeros(A, 7)
    anchors[:, 0] = ((cell % W).float() * 0.32).repeat_interleave(2)
    anchors[:, 1] = ((cell // W).float() * 0.32 - 39.68).repeat_interleave(2)
    anchors[:, 2] = -1.78
    anchors[:, 3:6] = torch.tensor([1.6, 3.9, 1.56])
    anchors[:, 6] = torch.tensor([0.0, math.pi / 2]).repeat(A // 2)
    anchors = anchors.to(dev)

    results = []
    for B in [int(v) for v in a.batches.split(",")]:
        for frac in [float(v) for v in a.fractions.split(",")]:
            g = torch.Generator().manual_seed(0)
            box = (0.15 * torch.randn(B, A, 7, generator=g)).to(dev)
            cls = -4.0 + 0.05 * torch.randn(B, A, 1, generator=g)
            hot = torch.rand(B, A, 1, generator=g) < frac
            cls = torch.where(hot, torch.rand(B, A, 1, generator=g) * 4.5 - 1.5, cls).to(dev)
            dirp = torch.randn(B, A, 2, generator=g).to(dev)
            kw = dict(num_class=1, nms_score_threshold=a.thresh, nms_pre_max_size=a.pre, nms_post_max_size=a.post, nms_iou_threshold=0.5)
            ws = torch.empty(D.workspace_bytes(B, A, 1, a.pre, a.post), dtype=torch.uint8, device=dev)
            out = {}
            for flavour, fused in (("fused", True), ("torch ops", False)):
                def step():
                    return D.predict_tensors(box, cls, dirp, anchors, fused=fused, workspace=ws if fused else None, out=out, **kw)

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
                row = {"batch": B, "hot_fraction": frac, "flavour": flavour, "launches_per_step": launches, "eager": spread(step),
                       "num_pass": r["num_pass"].tolist(), "num_det": r["num_det"].tolist()}
                if fused:
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
                    row["graph"] = "not captured: this flavour reads counts on the host"
                results.append(row)
    print(json.dumps({"op": "predict_tensors", "anchors": A, "pre_max": a.pre, "post_max": a.post, "score_thresh": a.thresh, "steps": a.steps,
                      "repeats": a.repeats, "results": results}))


if __name__ == "__main__":
    main()
