"""The summation orders of the partial-sum folds (papc_amd/csrc/fold.h), pinned bit for bit.

Every public fold entry point against a NumPy float32 emulation of the order fold.h documents.  A fold only adds, and a float32
NumPy add is the IEEE add the kernels perform, so the comparison is on the BITS of the result (int32 views: a flipped sign of a
zero fails too); no tolerance.  Most launch-structure tests of this suite compare two GPU paths with each other -- this one is what
says which order both of them must have.

The three orders (fold.h):
  lane fold      FW chunk lanes; lane l adds chunks l, l + FW, l + 2 FW, ... to 0.f in that order; lane 0 then adds the sums of lanes
                 1 .. FW - 1 in lane order.                                    papc_reduce_partials_f32 / 2 / _batch (FW = 16),
                 papc_reduce_partials2_f32's wide path (FW = 4), papc_fold_jobs_f32's scalar and float4 kinds (FW = PAPC_FOLD_WAVES)
  in-order fold  starts from chunk 0 (not from 0.f + chunk 0) and adds chunks 1, 2, ... in order.
                                                                               papc_fold_jobs_f32's wide kind, papc_pg_fold_f32
  slice tree     64 slices; slice s adds chunks s, s + 64, ... to 0.f in order; the slice sums are folded in a binary tree
                 (s += s + 32, then + 16, ... + 1).                            papc_reduce_partials_strided_f32
accumulate != 0 adds the fold's result to what `out` held, as the last add.
"""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib, folds
from papc_amd.smallm import PgFoldJob

pytestmark = pytest.mark.gpu


# ---- the orders, in NumPy float32 ------------------------------------------------------------------------------------------------
def lane_fold(part, fw):
    """part [n_chunks, n] float32 -> [n]"""
    lanes = np.zeros((fw, part.shape[1]), np.float32)
    for t in range(part.shape[0]):          # t ascending: every lane sees its chunks in order
        lanes[t % fw] += part[t]
    s = lanes[0].copy()
    for g in range(1, fw):
        s += lanes[g]
    return s


def in_order_fold(part, from_zero=False):
    s = np.zeros(part.shape[1], np.float32) + part[0] if from_zero else part[0].copy()
    for t in range(1, part.shape[0]):
        s += part[t]
    return s


def slice_tree_fold(part):
    sl = np.zeros((64, part.shape[1]), np.float32)
    for t in range(part.shape[0]):
        sl[t % 64] += part[t]
    h = 32
    while h >= 1:
        sl[:h] += sl[h:2 * h]
        h //= 2
    return sl[0].copy()


def finish(s, out0, acc):
    assert s.dtype == np.float32 and out0.dtype == np.float32
    return out0 + s if acc else s


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def values(rng, shape):
    """a wide exponent spread (a changed order changes bits), and a column of -0.0 (the sign of a zero depends on the start value)"""
    v = (rng.normal(size=shape) * 10.0 ** rng.uniform(-3, 3, size=shape)).astype(np.float32)
    v.reshape(shape[0], -1)[:, 1::17] = -0.0
    return v


def bits_equal(got, ref):
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    return torch.equal(got.detach().cpu().contiguous().view(torch.int32), torch.from_numpy(ref).view(torch.int32).reshape(got.shape))


def test_the_orders_differ_on_these_inputs():
    """The self-check of the inputs: had a kernel summed in another order, the comparisons below would see it."""
    part = values(np.random.default_rng(1234), (200, 1000))
    lane16 = lane_fold(part, 16)
    assert not np.array_equal(lane16, in_order_fold(part, from_zero=True)), "a plain sequential sum equals the 16-lane order on this input"
    assert not np.array_equal(lane16, lane_fold(part, 8)), "8 and 16 chunk lanes give the same bits on this input"
    assert not np.array_equal(lane16, slice_tree_fold(part))
    assert not np.array_equal(lane_fold(part[:37], 4), in_order_fold(part[:37]))
    # the start value: a chunk-0 start keeps a negative zero, a 0.f start does not
    z = np.full((1, 4), -0.0, np.float32)
    assert np.signbit(in_order_fold(z)).all() and not np.signbit(in_order_fold(z, from_zero=True)).any() and not np.signbit(lane_fold(z, 16)).any()


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n_chunks,n", [(200, 1000), (37, 50), (16, 64), (1, 5), (300, 129)])
def test_reduce_partials(dev, n_chunks, n, acc):
    rng = np.random.default_rng(100 + n_chunks)
    part, out0 = values(rng, (n_chunks, n)), values(rng, (1, n))[0]
    tp, to = torch.from_numpy(part).to(dev), torch.from_numpy(out0).to(dev)
    _lib.check(_lib.load().papc_reduce_partials_f32(tp.data_ptr(), n_chunks, n, to.data_ptr(), acc, _lib.stream_ptr()), "papc_reduce_partials_f32")
    torch.cuda.synchronize()
    ref = lane_fold(part, 16)
    if n_chunks > 16:       # (the input tells the orders apart: a plain sequential sum over the chunks has other bits)
        assert not np.array_equal(ref, in_order_fold(part, from_zero=True))
    assert bits_equal(to, finish(ref, out0, acc))


def _partials2(dev, n_chunks, n1, n2, pad, acc, fw, seed):
    rng = np.random.default_rng(seed)
    ld = n1 + n2 + pad
    part = values(rng, (n_chunks, ld))
    o1, o2 = values(rng, (1, n1))[0], values(rng, (1, max(n2, 1)))[0]
    tp, t1, t2 = torch.from_numpy(part).to(dev), torch.from_numpy(o1).to(dev), torch.from_numpy(o2).to(dev)
    _lib.check(_lib.load().papc_reduce_partials2_f32(tp.data_ptr(), n_chunks, ld, n1, t1.data_ptr(), n2, t2.data_ptr() if n2 else None, acc,
                                                     _lib.stream_ptr()), "papc_reduce_partials2_f32")
    torch.cuda.synchronize()
    s = lane_fold(part[:, :n1 + n2], fw)
    assert bits_equal(t1, finish(s[:n1], o1, acc))
    if n2:
        assert bits_equal(t2, finish(s[n1:], o2, acc))
    else:
        assert bits_equal(t2, o2)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n_chunks,n1,n2,pad", [(45, 300, 20, 10), (130, 61, 0, 0), (70, 16384, 128, 0), (8, 16384, 128, 3)])
def test_reduce_partials2_narrow(dev, n_chunks, n1, n2, pad, acc):
    """16 chunk lanes: few elements, or more than 64 chunks, or a chunk stride that is no multiple of 4"""
    _partials2(dev, n_chunks, n1, n2, pad, acc, 16, 200 + n_chunks)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n_chunks,n1,n2,pad", [(37, 16384, 128, 4), (5, 20000, 0, 0), (64, 16640, 12, 0)])
def test_reduce_partials2_wide(dev, n_chunks, n1, n2, pad, acc):
    """n_chunks <= 64, n1 + n2 >= 16384, n1, n2 and the chunk stride multiples of 4: 4 chunk lanes of float4"""
    assert n_chunks <= 64 and n1 + n2 >= 16384 and n1 % 4 == 0 and n2 % 4 == 0 and (n1 + n2 + pad) % 4 == 0
    _partials2(dev, n_chunks, n1, n2, pad, acc, 4, 300 + n_chunks)


@pytest.mark.parametrize("acc", [0, 1])
def test_reduce_partials_batch(dev, acc):
    rng = np.random.default_rng(400 + acc)
    specs = [(37, 300, 20, 10), (130, 1000, 0, 0), (3, 40, 7, 1)]      # (n_chunks, n1, n2, ld pad): the grid is as wide as the widest job
    jobs = (_lib.ReduceJob * len(specs))()
    keep = []
    for i, (nc, n1, n2, pad) in enumerate(specs):
        ld = n1 + n2 + pad
        part, o1, o2 = values(rng, (nc, ld)), values(rng, (1, n1))[0], values(rng, (1, max(n2, 1)))[0]
        tp, t1, t2 = torch.from_numpy(part).to(dev), torch.from_numpy(o1).to(dev), torch.from_numpy(o2).to(dev)
        keep.append((part, o1, o2, tp, t1, t2))
        jobs[i] = _lib.ReduceJob(tp.data_ptr(), nc, acc, ld, n1, n2, t1.data_ptr(), t2.data_ptr() if n2 else None)
    _lib.check(_lib.load().papc_reduce_partials_batch_f32(jobs, len(specs), _lib.stream_ptr()), "papc_reduce_partials_batch_f32")
    torch.cuda.synchronize()
    for (nc, n1, n2, pad), (part, o1, o2, tp, t1, t2) in zip(specs, keep):
        s = lane_fold(part[:, :n1 + n2], 16)
        assert bits_equal(t1, finish(s[:n1], o1, acc))
        assert bits_equal(t2, finish(s[n1:], o2, acc) if n2 else o2)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n_chunks,rows,cols,out_ld,pad", [(100, 37, 3, 7, 5), (300, 64, 3, 67, 0), (5, 1, 10, 10, 0), (64, 5, 16, 16, 2)])
def test_reduce_partials_strided(dev, n_chunks, rows, cols, out_ld, pad, acc):
    rng = np.random.default_rng(500 + n_chunks)
    ld = rows * cols + pad
    part, out0 = values(rng, (n_chunks, ld)), values(rng, (rows, out_ld))
    tp, to = torch.from_numpy(part).to(dev), torch.from_numpy(out0).to(dev)
    _lib.check(_lib.load().papc_reduce_partials_strided_f32(tp.data_ptr(), n_chunks, ld, rows, cols, to.data_ptr(), out_ld, acc, _lib.stream_ptr()),
               "papc_reduce_partials_strided_f32")
    torch.cuda.synchronize()
    ref = out0.copy()
    ref[:, :cols] = finish(slice_tree_fold(part[:, :rows * cols]).reshape(rows, cols), out0[:, :cols], acc)
    assert bits_equal(to, ref)


def _fold_kind(n_chunks, rows, cols, ld, out_ld):
    """which of its three shapes papc_fold_jobs_f32 runs a job in (16-byte aligned buffers)"""
    n = rows * cols
    contiguous = n % 4 == 0 and ld % 4 == 0 and (rows == 1 or out_ld == cols)
    if contiguous and n_chunks <= 16 and n >= 16384:
        return "wide"
    return "vec" if contiguous and n >= 1024 else "scalar"


@pytest.mark.parametrize("fw", [16, 8])
def test_fold_jobs(dev, fw):
    lib = _lib.load()
    rng = np.random.default_rng(600)
    specs = [  # (n_chunks, rows, cols, out_ld, ld pad, accumulate)
        (37, 128, 3, 131, 5, 1), (200, 1, 50, 50, 0, 0), (300, 1, 1026, 1026, 0, 1),                         # scalar
        (37, 1, 2048, 2048, 4, 0), (300, 16, 100, 100, 0, 1), (20, 1, 16384, 16384, 0, 0),                   # float4 lanes
        (7, 1, 16388, 16388, 0, 1), (16, 128, 129 * 4, 129 * 4, 8, 0), (1, 1, 20000, 20000, 0, 0)]           # wide
    kinds = [_fold_kind(nc, rows, cols, rows * cols + pad, out_ld) for nc, rows, cols, out_ld, pad, _ in specs]
    assert kinds == ["scalar"] * 3 + ["vec"] * 3 + ["wide"] * 3
    jobs = (folds.FoldJob * len(specs))()
    keep = []
    for i, (nc, rows, cols, out_ld, pad, acc) in enumerate(specs):
        ld = rows * cols + pad
        part, out0 = values(rng, (nc, ld)), values(rng, (rows, out_ld))
        tp, to = torch.from_numpy(part).to(dev), torch.from_numpy(out0).to(dev)
        keep.append((part, out0, tp, to))
        jobs[i] = folds.FoldJob(tp.data_ptr(), nc, acc, ld, rows, cols, to.data_ptr(), out_ld)
    old = ctypes.c_int(0)
    _lib.check(lib.papc_knob_get(b"PAPC_FOLD_WAVES", ctypes.byref(old)), "papc_knob_get")
    _lib.check(lib.papc_knob_set(b"PAPC_FOLD_WAVES", fw), "papc_knob_set")
    try:
        _lib.check(lib.papc_fold_jobs_f32(jobs, len(specs), _lib.stream_ptr()), "papc_fold_jobs_f32")
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.papc_knob_set(b"PAPC_FOLD_WAVES", old.value), "papc_knob_set")
    for i, ((nc, rows, cols, out_ld, pad, acc), kind, (part, out0, tp, to)) in enumerate(zip(specs, kinds, keep)):
        blk = part[:, :rows * cols]
        s = in_order_fold(blk) if kind == "wide" else lane_fold(blk, fw)
        ref = out0.copy()
        ref[:, :cols] = finish(s.reshape(rows, cols), out0[:, :cols], acc)
        assert bits_equal(to, ref), "job %d (%s, %d chunk lanes)" % (i, kind, fw)


@pytest.mark.parametrize("acc", [0, 1])
def test_pg_fold(dev, acc):
    rng = np.random.default_rng(700 + acc)
    specs = [(5, 4099, 4104), (1, 3, 4), (8, 1026, 1028)]       # (nsplit, n, stride): n % 4 != 0, the ragged tail runs
    jobs = (PgFoldJob * len(specs))()
    keep = []
    for i, (ns, n, stride) in enumerate(specs):
        assert n % 4 != 0 and stride % 4 == 0
        part, out0 = values(rng, (ns, stride)), values(rng, (1, n))[0]
        tp, to = torch.from_numpy(part).to(dev), torch.from_numpy(out0).to(dev)
        keep.append((part, out0, tp, to))
        jobs[i] = PgFoldJob(tp.data_ptr(), ns, stride, n, to.data_ptr(), acc)
    _lib.check(_lib.load().papc_pg_fold_f32(jobs, len(specs), _lib.stream_ptr()), "papc_pg_fold_f32")
    torch.cuda.synchronize()
    for (ns, n, stride), (part, out0, tp, to) in zip(specs, keep):
        assert bits_equal(to, finish(in_order_fold(part[:, :n]), out0, acc))
