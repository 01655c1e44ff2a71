"""The grouped plane-set GEMM (papc_pg_gemm_group_f32, csrc/smallm.hip): a layer's dX and split-K dW products in ONE launch must give
results BIT-identical to the two separate papc_pg_gemm_f32 launches (PAPC_PG_GROUP=0) -- the raw entry point, and every gradient of the
group_all stack (dW after the fold, dgamma / dbeta, the input gradient) through both orchestrations, eagerly and under graph replay."""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib, smallm
from papc_amd.mlp import StackSpec
from papc_amd.stack import SharedMLPStack
from papc_amd.synthetic import make_clouds
from tests.util import seeded_weights

pytestmark = pytest.mark.gpu


@pytest.fixture
def group_knob():
    lib = _lib.load()
    old = ctypes.c_int()
    _lib.check(lib.papc_knob_get(b"PAPC_PG_GROUP", ctypes.byref(old)), "papc_knob_get")

    def set_(v):
        _lib.check(lib.papc_knob_set(b"PAPC_PG_GROUP", int(v)), "papc_knob_set")
    yield set_
    set_(old.value)


def _planes(lib, m, dev):
    """[R, K] fp32 -> planes (contraction over K)"""
    R, K = m.shape
    buf = torch.empty(lib.papc_pg_planes_bytes(R, K), dtype=torch.uint8, device=dev)
    job = (smallm.PgWJob * 1)()
    job[0].src, job[0].row_stride, job[0].col_stride, job[0].R, job[0].K, job[0].planes = m.data_ptr(), K, 1, R, K, buf.data_ptr()
    _lib.check(lib.papc_pg_prep_weights_f32(job, 1, _lib.stream_ptr()), "papc_pg_prep_weights_f32")
    return buf


def _rand(rng, shape, dev):
    return torch.from_numpy((rng.normal(size=shape) * np.exp(rng.normal(size=shape))).astype(np.float32)).to(dev)


def _layer_products(dev, M, cin, cout, red, seed):
    """the two products of one backward layer on random operands: dX [M, cin] (RED epilogue with its sums, or a plain store) and the split-K
    dW partials [split, cout, cin]; returns (descriptor array, outputs, keep-alive)"""
    lib = _lib.load()
    rng = np.random.default_rng(seed)
    dy, wt, x = _rand(rng, (M, cout), dev), _rand(rng, (cin, cout), dev), _rand(rng, (M, cin), dev)
    pdy, pwt, pdyt, pxt = _planes(lib, dy, dev), _planes(lib, wt, dev), _planes(lib, dy.t().contiguous(), dev), _planes(lib, x.t().contiguous(), dev)
    split = smallm._split_for(cout, cin, M // 32)
    dx = torch.full((M, cin), float("nan"), device=dev)
    part = torch.full((split, cout, cin), float("nan"), device=dev)
    gs = (smallm.PgGemm * 2)()
    g = gs[0]
    g.epi, g.a, g.b, g.R1, g.R2, g.K = (smallm.EPI_RED if red else smallm.EPI_STORE), pdy.data_ptr(), pwt.data_ptr(), M, cin, cout
    g.c, g.ldc, g.split, g.family = dx.data_ptr(), cin, 1, smallm.K_BWD_DX
    outs, keep = [dx, part], [pdy, pwt, pdyt, pxt]
    if red:
        sums = torch.full((M // 128, 2, cin), float("nan"), device=dev)
        y_prev = _rand(rng, (M, cin), dev)
        cst = torch.from_numpy(rng.normal(size=(4, cin)).astype(np.float32)).to(dev)
        cst[1] = cst[1].abs() + 0.5                                       # invstd
        g.stats, g.y_prev = sums.data_ptr(), y_prev.data_ptr()
        g.mean, g.invstd, g.scale, g.shift = (cst[i].data_ptr() for i in range(4))
        outs.append(sums)
        keep += [y_prev, cst]
    w = gs[1]
    w.epi, w.a, w.b, w.R1, w.R2, w.K = smallm.EPI_STORE, pdyt.data_ptr(), pxt.data_ptr(), cout, cin, M
    w.c, w.ldc, w.split, w.split_stride, w.family = part.data_ptr(), cin, split, cout * cin, smallm.K_BWD_DW
    return gs, outs, keep


@pytest.mark.parametrize("M,cin,cout,red", [
    (4096, 512, 1024, True),      # SA3 layer 3 (dX with the BN-backward sums of layer 2)
    (4096, 256, 512, True),       # layer 2
    (4096, 256, 256, False),      # layer 1: the input gradient (plain store)
    (384, 43, 72, True),          # ragged: Cin not a multiple of 64, K = 72 not a multiple of 32
    (512, 259, 24, False),        # ragged, a dW product with more k stages per workgroup than its dX (it runs first)
    (384, 43, 24, True),          # ... the same ahead of a RED product
])
def test_group_entry_point_equals_two_launches(dev, group_knob, M, cin, cout, red):
    lib = _lib.load()
    st = _lib.stream_ptr()
    gs, outs, keep = _layer_products(dev, M, cin, cout, red, M + cin + cout)
    _lib.check(lib.papc_pg_gemm_f32(ctypes.byref(gs[0]), st), "papc_pg_gemm_f32")
    _lib.check(lib.papc_pg_gemm_f32(ctypes.byref(gs[1]), st), "papc_pg_gemm_f32")
    want = [t.clone() for t in outs]
    assert all(bool(torch.isfinite(t).all()) for t in want)
    group_knob(1)
    for order in ((0, 1), (1, 0)):        # either product may come first in the array
        for t in outs:
            t.fill_(float("nan"))
        arr = (smallm.PgGemm * 2)(gs[order[0]], gs[order[1]])
        _lib.check(lib.papc_pg_gemm_group_f32(arr, 2, st), "papc_pg_gemm_group_f32")
        for a, b in zip(outs, want):
            assert torch.equal(a, b), order
    # a lone product goes through as papc_pg_gemm_f32
    outs[1].fill_(float("nan"))
    _lib.check(lib.papc_pg_gemm_group_f32(ctypes.byref(gs[1]), 1, st), "papc_pg_gemm_group_f32")
    assert torch.equal(outs[1], want[1])
    torch.cuda.synchronize()
    del keep


def test_group_entry_point_rejects_pairs_it_cannot_launch(dev):
    lib = _lib.load()
    st = _lib.stream_ptr()
    gs, outs, keep = _layer_products(dev, 512, 64, 128, True, 3)
    two_red = (smallm.PgGemm * 2)(gs[0], gs[0])
    assert lib.papc_pg_gemm_group_f32(two_red, 2, st) == -2                      # PAPC_E_UNSUPPORTED
    fwd = (smallm.PgGemm * 2)(gs[0], gs[1])
    fwd[0].epi = smallm.EPI_FWD
    assert lib.papc_pg_gemm_group_f32(fwd, 2, st) == -2
    assert lib.papc_pg_gemm_group_f32(gs, 3, st) == -1 and lib.papc_pg_gemm_group_f32(None, 2, st) == -1
    torch.cuda.synchronize()
    del keep, outs


# (B, D, mlp, xyz_first): PointNet2_SSG_Clas.sa3 at the benchmark batch (M = 4096, 259 -> 256 -> 512 -> 1024), and a ragged stack
# (Cin = 43, K = 72 / 24: neither a multiple of 32 nor of 64)
SHAPES = [(32, 256, [256, 512, 1024], True), (3, 40, [48, 72, 24], False)]


def _stack_args(dev, B, D, mlp, xyz_first, seed):
    N = 128
    rng = np.random.default_rng(seed)
    xyz = torch.from_numpy(np.ascontiguousarray(make_clouds(B, N, seed).transpose(0, 2, 1))).to(dev)
    feats = torch.from_numpy(rng.normal(size=(B, N, D)).astype(np.float32)).to(dev)
    ws = seeded_weights([D + 3] + mlp, seed + 1)
    params = [torch.from_numpy(a).to(dev).requires_grad_(True) for tup in ws for a in tup]
    gout = torch.from_numpy(rng.normal(size=(B, mlp[-1])).astype(np.float32)).to(dev)
    return (StackSpec(B, N, 1, N, D, xyz_first), None, xyz, torch.zeros(B, 1, 3, device=dev)), feats.requires_grad_(True), params, gout


def _fwd_bwd(fn, head, feats, params, gout):
    out = fn.apply(*head, feats, None, None, *params)
    assert fn is not SharedMLPStack or out.grad_fn.planes       # (the library took the planes path)
    out.backward(gout)
    return [out.detach()] + [p.grad for p in params] + [feats.grad]


def _clear(feats, params):
    feats.grad = None
    for p in params:
        p.grad = None


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fn", [smallm.PlanesMLPMax, SharedMLPStack], ids=["python", "library"])
def test_stack_gradients_bit_identical(dev, group_knob, shape, fn):
    head, feats, params, gout = _stack_args(dev, *shape, seed=7)
    res = []
    for knob in (0, 1):
        group_knob(knob)
        _clear(feats, params)
        res.append([t.clone() for t in _fwd_bwd(fn, head, feats, params, gout)])
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(*res)):
        assert a is not None and torch.isfinite(a).all()
        assert torch.equal(a, b), "tensor %d (0 = output, then w / b / gamma / beta per layer, last = grad feats)" % i


def test_stack_graph_replay_bit_identical(dev, group_knob):
    head, feats, params, gout = _stack_args(dev, *SHAPES[0], seed=9)
    group_knob(0)
    _clear(feats, params)
    want = [t.clone() for t in _fwd_bwd(SharedMLPStack, head, feats, params, gout)]
    group_knob(1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _clear(feats, params)
        _fwd_bwd(SharedMLPStack, head, feats, params, gout)          # warm-up outside the capture
        _clear(feats, params)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            got = _fwd_bwd(SharedMLPStack, head, feats, params, gout)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for rep in range(2):
        for t in got:
            t.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), "replay %d, tensor %d" % (rep, i)


def test_grouped_launches_replace_the_pairs(dev, group_knob):
    """PAPC_PG_GROUP=1: the SA3 backward issues one grouped launch per layer and no separate backward planes GEMM"""
    from torch.profiler import ProfilerActivity, profile
    head, feats, params, gout = _stack_args(dev, *SHAPES[0], seed=11)
    counts = []
    for knob in (0, 1):
        group_knob(knob)
        _clear(feats, params)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            _fwd_bwd(SharedMLPStack, head, feats, params, gout)
            torch.cuda.synchronize()
        ev = prof.key_averages()
        counts.append((sum(e.count for e in ev if "pg_gemm_group_kernel" in e.key),
                       sum(e.count for e in ev if "pg_gemm_kernel" in e.key)))
    assert counts[0] == (0, 3 + 6), counts          # forward 3, backward dX 3 + dW 3
    assert counts[1] == (3, 3), counts
