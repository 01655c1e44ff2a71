"""The end of the step without the launches nothing waits for (include/papc_hip.h: PAPC_FOLD_F64Q, PAPC_FOLD_FIN; csrc/finalize.h).

With a fold list a stack's backward hands the float64 fold of the no-store max layer's dW partials to the step's deferred folds and the
two closed forms -- that layer's dW and the whole backward of the coordinates-only first layer -- to ONE finalize launch behind them
(PAPC_FOLD_FIN=1, the default) instead of three launches in the middle of the chain (=0).  The same sums in the same order and the same
float64 expressions per output element: every gradient buffer must come out BIT-identical, with fresh and with accumulating targets.

Likewise at the head of the step: the coordinates-only first layer's forward finalize as one extra workgroup of the weight transposes'
launch (papc_sa_mlp_xyz1_prep, PAPC_XYZ1_RIDE) leaves the bits the forward's own launch leaves.

The stack is SA1-shaped -- B = 2, S = 16, K = 32, widths [64, 64, 128] -- driven through the raw C entry points (torch only owns the
memory), with the chip-sized thresholds scaled down so that this shape takes the moment-path first layer and the no-store max layer."""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib, folds
from papc_amd import functional as F
from papc_amd.stack import SaDesc, SaGrads, SaIo, SaPlan
from papc_amd.synthetic import make_clouds, make_start_idx
from tests.util import seeded_weights

pytestmark = pytest.mark.gpu

KNOBS = ("PAPC_STREAM_MINTILES", "PAPC_GEMM_MINWG", "PAPC_FOLD_FIN", "PAPC_XYZ1_RIDE")


def _knob_get(name):
    v = ctypes.c_int(0)
    _lib.check(_lib.load().papc_knob_get(name.encode(), ctypes.byref(v)), "papc_knob_get")
    return v.value


def _knob(name, value):
    _lib.check(_lib.load().papc_knob_set(name.encode(), int(value)), "papc_knob_set")


@pytest.fixture
def knobs():
    old = {n: _knob_get(n) for n in KNOBS}
    _knob("PAPC_STREAM_MINTILES", 1)
    _knob("PAPC_GEMM_MINWG", 1)
    yield old
    for n, v in old.items():
        _knob(n, v)


B, N, S, K, CHANS = 2, 256, 16, 32, [3, 64, 64, 128]


@pytest.fixture(scope="module")
def sa1_inputs(dev):
    x = make_clouds(B, N, 5)
    xyz = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    st = torch.from_numpy(make_start_idx(B, N, 5)).to(dev)
    _, new_xyz = F._fps_raw(xyz, S, st)
    idx = F._ball_query_raw([0.4], [K], xyz, new_xyz)[0]
    rng = np.random.default_rng(8)
    gout = torch.from_numpy(rng.normal(size=(B * S, CHANS[-1])).astype(np.float32)).to(dev)
    return xyz, new_xyz, idx, seeded_weights(CHANS, 31), gout


def _sa1_plan(dev, inputs, xyz_pre=None):
    """descriptor, io and plan of the stack with fresh parameter and running-statistics tensors; (lib, io, plan, keep)"""
    lib = _lib.load()
    xyz, new_xyz, idx, ws, gout = inputs
    L = len(CHANS) - 1
    par = [[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in tup] for tup in ws]
    d = SaDesc()
    d.B, d.N, d.S, d.K, d.D, d.n_layers, d.cin = B, N, S, K, 0, L, 3
    for l in range(L):
        d.cout[l] = CHANS[l + 1]
    d.input, d.identity_rows, d.xyz_first, d.pool, d.eval_bn = 0, 0, 1, 1, 0
    d.eps, d.momentum = 1e-5, 0.9
    io = SaIo()
    io.xyz, io.sb, io.sn, io.sc = xyz.data_ptr(), xyz.stride(0), xyz.stride(1), xyz.stride(2)
    io.new_xyz, io.idx = new_xyz.data_ptr(), idx.data_ptr()
    c3 = torch.tensor([1.0, 0.0, 1e30], device=dev).view(3, 1).expand(3, 1024).contiguous()
    io.consts3, io.consts3_ld = c3.data_ptr(), 1024
    run = [(torch.zeros(CHANS[l + 1], device=dev), torch.ones(CHANS[l + 1], device=dev)) for l in range(L)]
    for l in range(L):
        io.layer[l].w, io.layer[l].b, io.layer[l].gamma, io.layer[l].beta = (t.data_ptr() for t in par[l])
        io.layer[l].running_mean, io.layer[l].running_var = (t.data_ptr() for t in run[l])
    if xyz_pre is not None:
        io.xc, io.xc_gram = xyz_pre[0].data_ptr(), xyz_pre[1].data_ptr()
    plan = SaPlan()
    _lib.check(lib.papc_sa_mlp_plan(ctypes.byref(d), ctypes.byref(io), ctypes.byref(plan)), "papc_sa_mlp_plan")
    assert plan.xyz1 and plan.nostore, "the stack must take the moment-path first layer and the no-store max layer"
    return lib, io, plan, (par, run, c3, xyz_pre)


def _sa1_backward(dev, inputs, acc, defer):
    """forward + backward of the stack; returns (gradient buffers per layer, the entries of the fold list as (rows, cols) or None)"""
    lib, io, plan, keep = _sa1_plan(dev, inputs)
    gout = inputs[4]
    L = len(CHANS) - 1
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty(B * S, CHANS[-1], device=dev)
    saved = torch.empty(plan.saved_bytes, device=dev, dtype=torch.uint8)
    scr = torch.empty(max(plan.fwd_scratch_bytes, plan.bwd_scratch_bytes), device=dev, dtype=torch.uint8)
    io.out, io.saved, io.scratch = out.data_ptr(), saved.data_ptr(), scr.data_ptr()
    _lib.check(lib.papc_sa_mlp_fwd(ctypes.byref(plan), ctypes.byref(io), st), "papc_sa_mlp_fwd")
    g = SaGrads()
    g.gout = gout.data_ptr()
    grads = []
    for l in range(L):
        cin = CHANS[l]
        t = [torch.empty(CHANS[l + 1], cin, device=dev), torch.empty(CHANS[l + 1], device=dev), torch.empty(CHANS[l + 1], device=dev),
             torch.empty(CHANS[l + 1], device=dev)]
        for j, x in enumerate(t):
            x.fill_(3.0 + 0.25 * j + l)
        g.dw[l], g.db[l], g.dgamma[l], g.dbeta[l] = (x.data_ptr() for x in t)
        g.acc_w[l] = g.acc_gb[l] = acc
        grads.append(t)
    jobs = (folds.FoldJob * folds.CAPACITY)()
    lst = folds.FoldList(ctypes.cast(jobs, ctypes.POINTER(folds.FoldJob)), folds.CAPACITY, 0)
    if defer:
        g.defer = ctypes.cast(ctypes.pointer(lst), ctypes.c_void_p)
    _lib.check(lib.papc_sa_mlp_bwd(ctypes.byref(plan), ctypes.byref(io), ctypes.byref(g), st), "papc_sa_mlp_bwd")
    entries = None
    if defer:
        entries, i = [], 0
        while i < lst.count:
            entries.append((jobs[i].rows, jobs[i].cols))
            i += 1 + (jobs[i].n_chunks if jobs[i].rows == folds.FOLD_FIN else 0)
        _lib.check(lib.papc_fold_jobs_f32(jobs, lst.count, st), "papc_fold_jobs_f32")
    torch.cuda.synchronize()
    return grads, entries


def _kinds(entries):
    return sorted(r for r, _ in entries if r < 0)


@pytest.mark.parametrize("acc", [0, 1])
def test_deferred_finalizes_leave_the_same_bits(dev, knobs, sa1_inputs, acc):
    """knob 0 against knob 1 with a fold list, and both against a backward without a list (which must take the old launches whatever the knob)"""
    _knob("PAPC_FOLD_FIN", 0)
    g0, e0 = _sa1_backward(dev, sa1_inputs, acc, defer=True)
    assert _kinds(e0) == [], "PAPC_FOLD_FIN=0 queued a finalize: %s" % (e0,)
    _knob("PAPC_FOLD_FIN", 1)
    g1, e1 = _sa1_backward(dev, sa1_inputs, acc, defer=True)
    # the max layer's float64 fold and the two closed forms (kind in cols: 1 = the max layer's dW, 2 = the coordinates-only layer)
    assert _kinds(e1) == [folds.FOLD_FIN, folds.FOLD_FIN, folds.FOLD_F64Q], e1
    assert sorted(c for r, c in e1 if r == folds.FOLD_FIN) == [1, 2], e1
    assert [e for e in e1 if e[0] > 0] == e0, "the float folds of the list changed"
    gn, en = _sa1_backward(dev, sa1_inputs, acc, defer=False)
    assert en is None
    for l in range(len(CHANS) - 1):
        for j, nm in enumerate(("w", "b", "gamma", "beta")):
            assert torch.isfinite(g1[l][j]).all(), (nm, l)
            assert torch.equal(g0[l][j], g1[l][j]), "d%s of layer %d: deferred finalizes differ from the launches inside the backward (acc %d)" % (nm, l, acc)
            assert torch.equal(gn[l][j], g1[l][j]), "d%s of layer %d: the fold list changed the bits (acc %d)" % (nm, l, acc)
    # the gradients were written at all (not the prefill), and accumulate added to the prefill
    assert not bool((g1[0][0] == 3.0).all()) and not bool((g1[2][0] == 5.0).all())
    if acc:
        fresh, _ = _sa1_backward(dev, sa1_inputs, 0, defer=True)
        for l in (0, 2):
            want = (3.0 + l) + fresh[l][0].double()
            assert float((g1[l][0].double() - want).abs().max()) <= 1e-6 * max(3.0 + l, float(fresh[l][0].abs().max()))


def test_a_full_list_falls_back_to_the_launches(dev, knobs, sa1_inputs):
    """a list without room for the records: the library launches the finalizes itself, same bits"""
    lib = _lib.load()
    _knob("PAPC_FOLD_FIN", 1)
    want, _ = _sa1_backward(dev, sa1_inputs, 0, defer=True)
    old = folds.CAPACITY
    folds.CAPACITY = 4        # the two float jobs of the middle layer fit, a finalize record (1 + FOLD_FIN_SLOTS slots behind them) does not
    try:
        got, entries = _sa1_backward(dev, sa1_inputs, 0, defer=True)
    finally:
        folds.CAPACITY = old
    assert _kinds(entries) == [], entries
    for l in range(len(CHANS) - 1):
        for j in range(4):
            assert torch.equal(want[l][j], got[l][j]), (l, j)
    assert lib.papc_abi_sizeof(b"papc_fold_fin") == ctypes.sizeof(folds.FoldFin)
    assert folds.FOLD_FIN_SLOTS * ctypes.sizeof(folds.FoldJob) >= ctypes.sizeof(folds.FoldFin)


def test_first_layer_finalize_rides_on_the_weight_transposes(dev, knobs, sa1_inputs):
    """papc_sa_mlp_xyz1_prep: the coordinates-only first layer's finalize as one extra workgroup of the transposes' launch (PAPC_XYZ1_RIDE=1)
    against the two launches (=0) and against the forward's own finalize: the layer-1 constants, the folded weights wf, the moments and the
    running statistics -- everything the call writes into `saved` -- and the stack's output are bit-equal, and so are the transposes."""
    from papc_amd.mlp import xyz_pregroup
    from papc_amd.stack import L1_DONE
    xyz, new_xyz, idx, ws, gout = sa1_inputs
    pre = xyz_pregroup(xyz, new_xyz, idx)
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(3)
    mats = [torch.from_numpy(rng.normal(size=sh).astype(np.float32)).to(dev) for sh in ((64, 64), (128, 64), (37, 50))]

    def run(mode, n_mats):
        lib, io, plan, keep = _sa1_plan(dev, sa1_inputs, xyz_pre=pre)
        saved = torch.zeros(plan.saved_bytes, device=dev, dtype=torch.uint8)
        scr = torch.empty(plan.fwd_scratch_bytes, device=dev, dtype=torch.uint8)
        out = torch.empty(B * S, CHANS[-1], device=dev)
        io.out, io.saved, io.scratch = out.data_ptr(), saved.data_ptr(), scr.data_ptr()
        dsts = [torch.zeros(m.shape[1], m.shape[0], device=dev) for m in mats[:n_mats]]
        after_prep = None
        if mode is not None:
            _knob("PAPC_XYZ1_RIDE", mode)
            n = n_mats
            srcs, dp = (ctypes.c_void_p * max(n, 1))(), (ctypes.c_void_p * max(n, 1))()
            lds, rws, cls, cps = ((ctypes.c_int * max(n, 1))() for _ in range(4))
            for i in range(n):
                srcs[i], dp[i], lds[i], rws[i], cls[i], cps[i] = mats[i].data_ptr(), dsts[i].data_ptr(), mats[i].shape[1], mats[i].shape[0], mats[i].shape[1], 0
            _lib.check(lib.papc_sa_mlp_xyz1_prep(ctypes.byref(plan), ctypes.byref(io), srcs, lds, dp, rws, cls, cps, n, st), "papc_sa_mlp_xyz1_prep")
            torch.cuda.synchronize()
            after_prep = saved.clone()
            plan.d.disable |= L1_DONE
        _lib.check(lib.papc_sa_mlp_fwd(ctypes.byref(plan), ctypes.byref(io), st), "papc_sa_mlp_fwd")
        torch.cuda.synchronize()
        cst = saved[plan.off_cst[0]: plan.off_cst[0] + 16 * CHANS[1]].view(torch.float32).clone()
        return dict(out=out, cst=cst, saved=saved, after_prep=after_prep, dsts=dsts, run=[t.clone() for t in keep[1][0]])

    own = run(None, 0)
    assert torch.isfinite(own["cst"]).all() and float(own["cst"].abs().max()) > 0
    for n_mats in (3, 0):
        two, ride = run(0, n_mats), run(1, n_mats)
        # everything the call wrote (constants, wf, moments: the rest of the zeroed buffer is untouched)
        assert torch.equal(two["after_prep"], ride["after_prep"]), "the riding finalize wrote other bits than the launch of its own"
        assert int(ride["after_prep"].ne(0).sum()) > 0
        for r in (two, ride):
            assert torch.equal(r["cst"], own["cst"]), "layer-1 constants differ from the forward's own finalize"
            assert torch.equal(r["saved"], own["saved"]), "the saved state of the forward differs"
            assert torch.equal(r["out"], own["out"])
            for a, b in zip(r["run"], own["run"]):
                assert torch.equal(a, b), "running statistics differ (updated twice, or not at all)"
            for m, t in zip(mats, r["dsts"]):
                assert torch.equal(t, m.t().contiguous()), "a transpose is wrong"

