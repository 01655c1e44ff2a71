"""Deferred folds (papc_amd/folds.py, papc_fold_jobs_f32): the partial reductions of a whole backward pass in one launch.

(i) the kernel against numpy on both of its shapes (many chunks / few chunks), strided outputs, accumulation -- and with jobs that share an
output, which must apply in list order;
(ii) a training step of PointNet2_SSG_Clas (reference: PAPC/models/classify/pointnet2/pointnet2.py:6-41, loop PAPC/train.py:106-116)
with the folds deferred against the same step with every stack folding its own partials: identical losses, gradients equal up to
the summation order of the strided / split-K jobs (the dW / db jobs keep their order and are bit-identical);
(iii) the same inside a captured hipGraph."""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib, folds
from papc_amd.distributed import FlatParams
from papc_amd.head import softmax_cross_entropy
from papc_amd.models import PointNet2_SSG_Clas
from papc_amd.synthetic import make_clouds, make_labels, make_start_idx
from tests.util import assert_close

pytestmark = pytest.mark.gpu


def test_fold_jobs_kernel_vs_numpy(dev):
    lib = _lib.load()
    rng = np.random.default_rng(5)
    specs = [  # (n_chunks, rows, cols, out_ld, ld pad, accumulate)
        (200, 1, 64 * 3, 64 * 3, 0, 0), (37, 128, 3, 131, 5, 1), (512, 1, 77, 77, 0, 1), (8, 1, 1024 * 512, 1024 * 512, 0, 1),
        (3, 1, 16384 + 4, 16384 + 4, 0, 0), (1, 1, 20000, 20000, 0, 0), (64, 64, 128, 200, 64, 0), (16, 1, 256 * 128, 256 * 128, 128, 1)]
    jobs = (folds.FoldJob * len(specs))()
    keep, refs = [], []
    for i, (nc, rows, cols, out_ld, pad, acc) in enumerate(specs):
        ld = rows * cols + pad
        part = rng.normal(size=(nc, ld)).astype(np.float32)
        out0 = rng.normal(size=(rows, out_ld)).astype(np.float32)
        tp, to = torch.from_numpy(part).to(dev), torch.from_numpy(out0).to(dev)
        keep += [tp, to]
        ref = out0.astype(np.float64).copy()
        blk = part[:, :rows * cols].astype(np.float64).sum(0).reshape(rows, cols)
        ref[:, :cols] = (ref[:, :cols] if acc else 0.0) + blk
        refs.append((to, ref, cols))
        jobs[i] = folds.FoldJob(tp.data_ptr(), nc, acc, ld, rows, cols, to.data_ptr(), out_ld)
    _lib.check(lib.papc_fold_jobs_f32(jobs, len(specs), _lib.stream_ptr()), "papc_fold_jobs_f32")
    torch.cuda.synchronize()
    for i, (to, ref, cols) in enumerate(refs):
        got = to.cpu().numpy()
        assert_close(got[:, :cols], ref[:, :cols], 2e-6, "fold job %d" % i)
        assert np.array_equal(got[:, cols:], ref[:, cols:].astype(np.float32)), "job %d wrote outside its block" % i


FOLD_MAX = 24      # include/papc_hip.h: PAPC_FOLD_MAX, the jobs of one launch

# Jobs that share ONE output buffer of 20 000 floats: (n_chunks, rows, cols, out_ld, first element, accumulate).  Every shape of the kernel
# (csrc/folds.hip: papc_fold_jobs_f32 picks wide for n_chunks <= 16 and n >= 16384, the float4 lane fold for other contiguous n >= 1024,
# else the lane fold), the same pointer twice in each of them, two strided column blocks that overlap in 12 of their 24 columns, and one
# overwriting job between the two wide ones, so that any other order than the list's gives other values.
_SHARING = [(4, 1, 16384, 16384, 0, 1),         # wide
            (40, 1, 2048, 2048, 1024, 1),       # float4 lane fold
            (37, 32, 24, 100, 515, 1),          # lane fold, a strided column block ...
            (37, 32, 24, 100, 527, 1),          # ... and the block 12 columns to its right
            (40, 1, 2048, 2048, 1024, 1),       # the float4 job's pointer again
            (37, 1, 77, 77, 5, 1),              # lane fold
            (3, 1, 300, 300, 6000, 0),          # overwrites what the jobs before it left there
            (37, 1, 77, 77, 5, 1),              # the lane job's pointer again
            (4, 1, 16384, 16384, 0, 1)]         # the wide job's pointer again
_PRIVATE = [(64, 1, 192, 192, 0), (37, 16, 3, 19, 1), (8, 1, 1024, 1024, 0), (100, 1, 77, 77, 1)]      # (n_chunks, rows, cols, out_ld, accumulate)
_NSHARED = 20000


def _overlapping_jobs(total):
    """``total`` jobs in list order: the sharing ones spread evenly, jobs on private outputs between them -> [(spec, private?)]"""
    at = sorted({int(v) for v in np.round(np.linspace(0, total - 1, len(_SHARING)))})
    assert len(at) == len(_SHARING)
    order, k, f = [], 0, 0
    for i in range(total):
        if i in at:
            order.append((_SHARING[k], False))
            k += 1
        else:
            order.append((_PRIVATE[f % len(_PRIVATE)], True))
            f += 1
    return order


def _run_overlapping(dev, order, seed):
    lib = _lib.load()
    rng = np.random.default_rng(seed)
    shared0 = rng.normal(size=_NSHARED).astype(np.float32)
    shared = torch.from_numpy(shared0).to(dev)
    ref_shared = shared0.astype(np.float64)
    jobs = (folds.FoldJob * len(order))()
    keep, outs = [shared], [(shared, ref_shared)]
    for i, (spec, private) in enumerate(order):
        nc, rows, cols, out_ld = spec[:4]
        off, acc = (0, spec[4]) if private else (spec[4], spec[5])
        part = rng.normal(size=(nc, rows * cols)).astype(np.float32)
        tp = torch.from_numpy(part).to(dev)
        keep.append(tp)
        if private:
            out0 = rng.normal(size=rows * out_ld).astype(np.float32)
            to, ref = torch.from_numpy(out0).to(dev), out0.astype(np.float64)
            outs.append((to, ref))
        else:
            to, ref = shared, ref_shared
        idx = off + np.arange(rows)[:, None] * out_ld + np.arange(cols)[None, :]
        assert idx.max() < ref.size
        blk = part.astype(np.float64).sum(0).reshape(rows, cols)
        ref[idx] = (ref[idx] if acc else 0.0) + blk                      # float64, applied in list order
        jobs[i] = folds.FoldJob(tp.data_ptr(), nc, acc, rows * cols, rows, cols, to.data_ptr() + 4 * off, out_ld)
    _lib.check(lib.papc_fold_jobs_f32(jobs, len(order), _lib.stream_ptr()), "papc_fold_jobs_f32")
    torch.cuda.synchronize()
    return [(to.cpu().numpy(), ref) for to, ref in outs], shared0


@pytest.mark.parametrize("total", [11, 40])
def test_fold_jobs_with_overlapping_outputs_apply_in_list_order(dev, total):
    """Accumulate jobs that share an output (a module applied twice inside one backward pass queues two jobs on one .grad): the result is the
    float64 sum applied in LIST order at the bar of test_fold_jobs_kernel_vs_numpy (2e-6: each job is the same fold, and a job adds one fp32
    rounding of the running value), with fewer and with more jobs than one launch takes (PAPC_FOLD_MAX = 24), and two calls on the same inputs
    are bit-identical.  (The jobs of one launch run concurrently: before papc_fold_jobs_f32 split its launches at overlapping outputs, two
    such jobs raced on the read-modify-write and one contribution was lost.)"""
    assert (total < FOLD_MAX) == (total == 11)
    order = _overlapping_jobs(total)
    res1, shared0 = _run_overlapping(dev, order, 17)
    res2, _ = _run_overlapping(dev, order, 17)
    for i, ((got, ref), (again, _)) in enumerate(zip(res1, res2)):
        assert np.array_equal(got, again), "output %d differs between two calls on the same inputs" % i
        assert_close(got, ref, 2e-6, "overlapping fold jobs, output %d of %d jobs" % (i, total))
    got = res1[0][0]
    assert np.array_equal(got[16384:], shared0[16384:]), "a job wrote behind the shared blocks"


def _step(dev, defer, graph):
    old = folds.ENABLED
    folds.ENABLED = defer
    try:
        B, N = 4, 1024
        torch.manual_seed(11)
        model = PointNet2_SSG_Clas(num_classes=16).to(dev).train()
        model.drop1.p = model.drop2.p = 0.0
        flat = FlatParams(model)
        x = torch.from_numpy(make_clouds(B, N, 3)).to(dev)
        y = torch.from_numpy(make_labels(B, 16, 3)).reshape(-1).to(dev)
        st = (torch.from_numpy(make_start_idx(B, N, 3)).to(dev), torch.from_numpy(make_start_idx(B, 512, 4)).to(dev))
        one = torch.ones((), device=dev)

        def fwd_bwd():
            loss = softmax_cross_entropy(model(x, st), y)
            loss.backward(one)
            return loss

        if graph:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                fwd_bwd()
                flat.zero_grad()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    loss = fwd_bwd()
                flat.zero_grad()
                g.replay()
            torch.cuda.current_stream().wait_stream(s)
        else:
            flat.zero_grad()
            loss = fwd_bwd()
        torch.cuda.synchronize()
        return float(loss), flat.grad.detach().cpu().numpy().copy()
    finally:
        folds.ENABLED = old


def test_deferred_folds_equal_per_stack_folds(dev):
    l0, g0 = _step(dev, False, False)
    for graph in (False, True):
        l1, g1 = _step(dev, True, graph)
        assert l0 == l1, (l0, l1)
        # (the gather-add backward's float atomics make two runs differ in the last bits whatever the fold does)
        assert_close(g1, g0, 2e-5, "flat gradient, deferred vs per-stack folds (graph=%s)" % graph)
    assert np.abs(g0).max() > 0


def test_failed_backward_leaves_no_stale_fold_jobs(dev):
    """A backward that raises after a stack has queued its folds (here: a hook on l2_points, i.e. behind SA3's backward) never runs the
    engine's final callbacks.  The NEXT pass must fold exactly its own jobs: gradients equal the per-stack-fold result (round-5 advisor
    finding: the armed thread-local list kept the stale jobs and skipped the registration of every later pass)."""
    l0, g0 = _step(dev, False, False)
    old = folds.ENABLED
    folds.ENABLED = True
    try:
        B, N = 4, 1024
        torch.manual_seed(11)
        model = PointNet2_SSG_Clas(num_classes=16).to(dev).train()
        model.drop1.p = model.drop2.p = 0.0
        flat = FlatParams(model)
        x = torch.from_numpy(make_clouds(B, N, 3)).to(dev)
        y = torch.from_numpy(make_labels(B, 16, 3)).reshape(-1).to(dev)
        st = (torch.from_numpy(make_start_idx(B, N, 3)).to(dev), torch.from_numpy(make_start_idx(B, 512, 4)).to(dev))
        one = torch.ones((), device=dev)

        def boom(g):
            raise RuntimeError("injected failure behind SA3's backward")

        tap = {}
        loss = softmax_cross_entropy(model(x, st, tap=tap), y)
        tap["l2_points"].register_hook(boom)
        with pytest.raises(RuntimeError, match="injected"):
            loss.backward(one)
        torch.cuda.synchronize()
        assert len(folds._live) == 1 and next(iter(folds._live.values())).lst.count > 0     # the failed pass's jobs were never folded
        flat.zero_grad()
        loss = softmax_cross_entropy(model(x, st), y)
        loss.backward(one)
        torch.cuda.synchronize()
        assert float(loss) == l0
        assert_close(flat.grad.detach().cpu().numpy(), g0, 2e-5, "flat gradient of the pass after a failed one")
    finally:
        folds.ENABLED = old
        folds._live.clear()
