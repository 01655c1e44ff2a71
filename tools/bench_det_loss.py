"""Time the PointPillars detection loss (papc_amd.detloss.pointpillars_loss), forward + backward, on the fused node and in torch ops.

    python tools/bench_det_loss.py [--batches 2,4] [--anchors 107136] [--classes 1] [--steps 50] [--warmup 10] [--repeats 5]

Step = the result dict + the three gradients (torch.autograd.grad seeded with head.unit_gradient), with the direction term on, at the KITTI
car config's A = 248 x 216 x 2 anchors.  Three flavours in one process on the same random inputs: ``fused`` (csrc/detloss.hip, what
PAPC_DET_LOSS=1 selects) with the per-anchor cls_loss / loc_loss of the reference's dict, ``fused, no per-anchor losses`` (the trainer's call)
and ``torch ops`` (PAPC_DET_LOSS=0).  Every step is timed with device events, eagerly and as a captured hipGraph replay; a figure is the
median of ``repeats`` timings of ``steps`` steps, min and max the run-to-run spread.  ``launches`` counts the device kernels of one eager
step (torch profiler).  Reads nothing outside the repository.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2,4")
    ap.add_argument("--anchors", type=int, default=107136)
    ap.add_argument("--classes", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()

    import torch
    from torch.profiler import ProfilerActivity, profile
    from papc_amd import detloss as D
    from papc_amd import head as H

    dev = torch.device("cuda:0")
    one = H.unit_gradient(dev)

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

    results = []
    A, C = a.anchors, a.classes
    for B in [int(v) for v in a.batches.split(",")]:
        g = torch.Generator().manual_seed(0)
        tgt = torch.randn(B, A, 7, generator=g)
        box = (tgt + 0.3 * torch.randn(B, A, 7, generator=g)).to(dev).requires_grad_()
        cls = (3 * torch.randn(B, A, C, generator=g)).to(dev).requires_grad_()
        dirp = torch.randn(B, A, 2, generator=g).to(dev).requires_grad_()
        labels = torch.randint(-1, 1, (B, A), generator=g)
        labels[torch.rand(B, A, generator=g) < 1e-3] = 1                     # about 100 positive anchors per sample
        labels, tgt, anchors = labels.to(dev), tgt.to(dev), torch.randn(B, A, 7, generator=g).to(dev)
        for flavour, fused, per_anchor in (("fused", True, True), ("fused, no per-anchor losses", True, False), ("torch ops", False, True)):
            def step():
                r = D.pointpillars_loss(box, cls, dirp, labels, tgt, anchors, num_class=C, fused=fused, per_anchor_losses=per_anchor)
                return r, torch.autograd.grad(r["loss"], (box, cls, dirp), grad_outputs=one)

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
            eager = spread(step)
            graph = torch.cuda.CUDAGraph()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                with torch.cuda.graph(graph, stream=s):
                    keep = step()
            torch.cuda.current_stream().wait_stream(s)
            timed(graph.replay, a.warmup)
            results.append({"batch": B, "flavour": flavour, "launches_per_step": launches, "eager": eager, "graph": spread(graph.replay),
                            "loss": round(float(keep[0]["loss"]), 6)})
            del graph, keep
    print(json.dumps({"op": "pointpillars_loss", "anchors": A, "classes": C, "direction": True, "steps": a.steps, "repeats": a.repeats,
                      "results": results}))


if __name__ == "__main__":
    main()
