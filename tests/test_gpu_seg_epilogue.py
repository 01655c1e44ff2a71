"""The ragged-group extremum epilogue of the compacted max layer (csrc/mlp_stream.hip, SG flavour) and its select kernel (csrc/compact.hip).

The compacted stack's last forward keeps, per (group, channel), a packed {ordered value : 0xFFFFFFFF - row} key combined by a 64-bit integer
atomic max across tiles, waves and workgroups; papc_bn_relu_select_seg_f32 turns the keys into out / argmax / ysel.  The pair replaces
papc_bn_relu_max_seg_f32's pass over the stored output and must give ITS bits: every comparison here is an integer equality against that
kernel run on the same stored y, or against the same call with PAPC_SEG_EPI=0.  No tolerance anywhere.

Shapes: Cin = 128, Cout = 256 (the flavour's widths), 40 ragged groups on 1 392 physical rows rounded up to 1 408 -- 44 tiles of 32 rows on six
workgroups per column block, every wave of a workgroup owns one.  At that size no wave sees a second tile (the launch grows with the row
capacity), so one case runs 2 048 groups on 74 112 rows: 2 316 tiles on 1 024 waves, two or three trips through a wave's tile loop."""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import compact as C
from papc_amd import functional as F
from papc_amd import stack as ST
from papc_amd.synthetic import make_clouds, make_start_idx
from tests.util import seeded_weights

pytestmark = pytest.mark.gpu

CIN, COUT, K = 128, 256, 64
A_BNRELU = 1


@pytest.fixture(autouse=True)
def _small_shapes_stream():
    """the row-streaming kernels normally start at 2 048 tiles; the test shapes are a few dozen"""
    lib = _lib.load()
    old = ctypes.c_int(0)
    _lib.check(lib.papc_knob_get(b"PAPC_STREAM_MINTILES", ctypes.byref(old)), "papc_knob_get")
    _lib.check(lib.papc_knob_set(b"PAPC_STREAM_MINTILES", 1), "papc_knob_set")
    yield
    _lib.check(lib.papc_knob_set(b"PAPC_STREAM_MINTILES", old.value), "papc_knob_set")


class _seg_epi:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        lib = _lib.load()
        self.old = ctypes.c_int(0)
        _lib.check(lib.papc_knob_get(b"PAPC_SEG_EPI", ctypes.byref(self.old)), "papc_knob_get")
        _lib.check(lib.papc_knob_set(b"PAPC_SEG_EPI", self.v), "papc_knob_set")

    def __exit__(self, *a):
        _lib.check(_lib.load().papc_knob_set(b"PAPC_SEG_EPI", self.old.value), "papc_knob_set")


# ---- a hand-made compact layout ------------------------------------------------------------------------------------------------------------------
def _layout(G=40):
    """40 groups, multiples of 8 rows: [0, 8) a group of exactly 8 rows; [24, 72) spans tiles 0, 1 and 2; [72, 96) ends ON a tile boundary and
    [96, 128) is a whole tile; the random rest puts boundaries at every segment position; the last group takes the rows rounding up to 128.
    (G = 2 048: the same on some 70 000 rows -- more tiles than the launch has waves, so a wave runs its tile loop more than once.)"""
    rng = np.random.default_rng(1 if G == 40 else 6)
    sizes = [8, 16, 48, 24, 32] + [int(8 * rng.integers(1, 9)) for _ in range(G - 5)]
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    total = int(start[-1])
    rows = (total + 127) // 128 * 128
    assert (1000 <= total <= 1600 if G == 40 else rows // 32 > 2 * 1024) and 0 < rows - total <= K - sizes[-1], (total, rows)
    assert 8 in sizes and any(s0 // 32 + 2 <= (s1 - 1) // 32 for s0, s1 in zip(start[:-1], start[1:]))
    assert any(s % 32 == 0 for s in start[1:-1]) and {int(s) % 32 for s in start[1:-1]} == {0, 8, 16, 24}
    seg = np.repeat(np.arange(G, dtype=np.int32), np.asarray(sizes) // 8)
    seg = np.concatenate([seg, np.full((rows - total) // 8, G - 1, np.int32)])
    wrow = np.ones(rows, np.float32)
    for g in range(G):
        n = sizes[g] + (rows - total if g == G - 1 else 0)
        wrow[start[g]] = 1.0 + (K - n)
    return dict(G=G, start=start, total=total, rows=rows, seg=seg, wrow=wrow, sizes=sizes)


CASES = ["plain", "ties", "zero_w", "huge", "nan", "many_tiles"]


def _inputs(case, lay):
    """(x [rows, CIN], previous layer's scale / shift, w, bias, gamma, beta): the hard cases are made THROUGH the GEMM"""
    rng = np.random.default_rng(17)
    rows, start, total, G = lay["rows"], lay["start"], lay["total"], lay["G"]
    x = rng.normal(size=(rows, CIN)).astype(np.float32)
    psc = rng.uniform(0.5, 1.5, CIN).astype(np.float32) * rng.choice([1.0, -1.0], CIN).astype(np.float32)
    psh = (rng.normal(size=CIN) * 0.3).astype(np.float32)
    (w, b, gamma, beta), = seeded_weights([CIN, COUT], 23)
    gamma[::7] = 0.0                                                   # (seeded_weights: a quarter of the channels negative; every seventh: zero)
    gamma[3] = -0.0
    if case == "ties":
        x[40] = x[30]                                                  # group [24, 72): the same row on both sides of the tile boundary at 32
        x[42] = x[41]                                                  # ... and twice in one tile
        x[start[7] + 5] = x[start[7] + 1]                              # both halves of one 8-row segment
        g3 = 20
        x[start[g3]:start[g3 + 1]] = x[start[g3]]                      # a whole group of identical rows: every channel ties everywhere
    if case == "zero_w":
        # a zero weight row: every row of the channel equals the bias -- ties across tiles, waves and workgroups; bias +0 / -0: the signed-zero case
        # (0 + (-0) = +0 out of the accumulator, so the stored zeros are +0 and the sign flip of a gamma < 0 channel makes the compared key -0)
        w[0:12] = 0.0
        b[0:12] = np.array([0.0, -0.0, 1.5, -2.5, 0.0, -0.0, 1e-40, -1e-40, 0.0, -0.0, 3.0, -3.0], np.float32)
        gamma[0:12] = np.array([1.0, 1.0, 1.0, 1.0, -1.0, -1.0, 1.0, -1.0, 0.0, 0.0, -1.0, -1.0], np.float32)
        w[12:16] = 0.0
        w[12:16, 0] = np.float32(2.0 ** -125)                          # a normal weight times an activation below 1/16: outputs in the denormal range, row by row
        b[12:16] = 0.0
        psc[0], psh[0] = 2.0 ** -6, 2.0 ** -7
        gamma[12:16] = np.array([1.0, -1.0, 1.0, -1.0], np.float32)
    if case == "huge":
        for r in (3, 29, 33, start[9] + 2, start[15], total - 1):      # rows of huge magnitude: 128 products of 1e38 overflow wherever the weights agree in sign
            x[r] = 1.0e38
        psc[:], psh[:] = 1.0, 0.0
        w[20], w[21] = 0.5, -0.5                                       # +inf and -inf for certain, in several groups, tiles and both half-waves
        gamma[20:24] = np.array([1.0, 1.0, -1.0, -1.0], np.float32)
        w[22], w[23] = 0.5, -0.5
    if case == "nan":
        for r in (5, 31, 32, start[11] + 7):                           # an infinite activation: inf - inf and inf * 0 -> NaN in every channel of the row
            x[r, 0] = np.inf
        g4 = 13
        x[start[g4]:start[g4 + 1], 0] = np.inf                         # a group of nothing but NaN
        psc[0], psh[0] = 1.0, 0.0
        w[5] = 0.0                                                     # (inf * 0)
    x[total:] = x[start[G - 1]]                                        # the rounding rows are copies of the last group's first row (compact.hip)
    return x, psc, psh, w, b, gamma, beta


def _run_pair(dev, lay, x, psc, psh, w, b, gamma, beta, scale_mode):
    lib = _lib.load()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows, G = lay["rows"], lay["G"]
    xd, pscd, pshd, wd, bd, gd, btd = (t(a) for a in (x, psc, psh, w, b, gamma, beta))
    startd, segd, wrowd = t(lay["start"]), t(lay["seg"]), t(lay["wrow"])
    rowsd = t(np.array([rows, lay["total"]], np.int32))
    parts = lib.papc_mlp_gemm_parts(rows)
    st = _lib.stream_ptr()
    assert lib.papc_mlp_seg_epi_ok(rows, CIN, COUT) == 1
    y0 = torch.full((rows, COUT), 7.0, device=dev)
    y1 = torch.full((rows, COUT), 9.0, device=dev)
    s0 = torch.full((parts, 2, COUT), 7.0, device=dev)
    s1 = torch.full((parts, 2, COUT), 9.0, device=dev)
    keys = torch.zeros(G * COUT, dtype=torch.int64, device=dev)
    _lib.check(lib.papc_mlp_gemm_rows_w_f32(A_BNRELU, xd.data_ptr(), CIN, None, pscd.data_ptr(), pshd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rows, CIN, COUT,
                                            y0.data_ptr(), s0.data_ptr(), None, rowsd.data_ptr(), wrowd.data_ptr(), st), "plain forward")
    _lib.check(lib.papc_mlp_gemm_rows_keys_f32(xd.data_ptr(), CIN, pscd.data_ptr(), pshd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rows, CIN, COUT,
                                               y1.data_ptr(), s1.data_ptr(), rowsd.data_ptr(), wrowd.data_ptr(), segd.data_ptr(), gd.data_ptr(),
                                               keys.data_ptr(), st), "keys forward")
    cst = torch.empty(4, COUT, device=dev)
    if scale_mode == "bn":      # the layer's own statistics: NaN / zero scales wherever a channel overflowed
        _lib.check(lib.papc_bn_finalize_f32(s1.data_ptr(), parts, G * K, COUT, gd.data_ptr(), btd.data_ptr(), 1e-5, 0.9, *_lib.cst_ptrs(cst), None, None, st),
                   "bn_finalize")
    else:                       # finite constants with the weight's sign: the keys decide every channel, +-inf included
        cst[2] = gd * 0.75
        cst[3] = btd
    res = []
    for which in (0, 1):
        out = torch.full((G, COUT), 5.0, device=dev)
        am = torch.full((G, COUT), -5, dtype=torch.int32, device=dev)
        ys = torch.full((G, COUT), 5.0, device=dev)
        if which == 0:
            _lib.check(lib.papc_bn_relu_max_seg_f32(y1.data_ptr(), COUT, startd.data_ptr(), cst[2].data_ptr(), cst[3].data_ptr(), G, out.data_ptr(),
                                                    am.data_ptr(), ys.data_ptr(), st), "seg_max")
        else:
            _lib.check(lib.papc_bn_relu_select_seg_f32(keys.data_ptr(), y1.data_ptr(), COUT, startd.data_ptr(), gd.data_ptr(), cst[2].data_ptr(),
                                                       cst[3].data_ptr(), G, out.data_ptr(), am.data_ptr(), ys.data_ptr(), st), "select")
        res.append((out, am, ys))
    torch.cuda.synchronize()
    return y0, s0, y1, s1, res, cst


def _bits(a):
    return a.contiguous().view(torch.int32)


@pytest.mark.parametrize("scale_mode", ["bn", "finite"])
@pytest.mark.parametrize("case", CASES)
def test_keys_and_select_give_seg_max_bits(dev, case, scale_mode):
    """forward with keys + select == papc_bn_relu_max_seg_f32 on the y that forward stored: out, argmax, ysel as integers; y and the statistics
    partials bit-identical to the plain compacted forward"""
    lay = _layout(2048 if case == "many_tiles" else 40)
    x, psc, psh, w, b, gamma, beta = _inputs(case, lay)
    y0, s0, y1, s1, ((o0, a0, z0), (o1, a1, z1)), cst = _run_pair(dev, lay, x, psc, psh, w, b, gamma, beta, scale_mode)
    rows = lay["rows"]
    assert torch.equal(_bits(y1[:rows]), _bits(y0[:rows])), "the stored output changed"
    assert torch.equal(_bits(s1), _bits(s0)), "the statistics partials changed"
    yh = y1.cpu().numpy()
    if case == "huge":
        assert np.isposinf(yh[[3, 29, 33]][:, [20, 22]]).all() and np.isneginf(yh[[3, 29, 33]][:, [21, 23]]).all()
    if case == "nan":
        g4 = 13
        assert np.isnan(yh[lay["start"][g4]:lay["start"][g4 + 1]]).all() and np.isnan(yh[5]).all()
    if case == "zero_w":
        assert (yh[:lay["total"], 0] == 0).all() and (np.abs(yh[:lay["total"], 12]) < 1.1754944e-38).all()       # zeros; nothing normal in the tiny channel
        print("distinct values in the denormal-range channel:", len(np.unique(yh[:lay["total"], 12])))
    if scale_mode == "finite":
        sc = cst[2].cpu().numpy()
        assert ((sc < 0) == (gamma < 0)).all() and np.isfinite(sc).all()      # no channel takes the select kernel's scan
    bad = (a0 != a1).nonzero()
    assert torch.equal(a1, a0), "argmax differs at (group, channel) %s: %s vs %s" % (bad[:4].tolist(), a1[a0 != a1][:4].tolist(), a0[a0 != a1][:4].tolist())
    assert torch.equal(_bits(z1), _bits(z0)), "ysel differs"
    assert torch.equal(_bits(o1), _bits(o0)), "out differs"
    am = a0.cpu().numpy()
    st = lay["start"]
    assert ((am >= st[:-1, None]) & (am < st[1:, None])).all()
    if case == "nan" and scale_mode == "finite":
        g4 = 13
        assert (am[g4] == st[g4]).all() and np.isinf(z0.cpu().numpy()[g4]).all()       # a group of nothing but NaN: its first row and -+inf


def test_unbuilt_widths_are_refused_and_seg_max_stays(dev):
    """a width pair without the flavour: the query says no, the entry point fails loudly (no quiet fall-back), and papc_bn_relu_max_seg_f32 on such a
    layer is still the exact first-row extremum"""
    lib = _lib.load()
    lay = _layout()
    rows, G = lay["rows"], lay["G"]
    assert lib.papc_mlp_seg_epi_ok(rows, 64, 128) == 0 and lib.papc_mlp_seg_epi_ok(rows, 128, 192) == 0 and lib.papc_mlp_seg_epi_ok(rows + 32, CIN, COUT) == 0
    z = torch.zeros(rows * 128, device=dev)
    rc = lib.papc_mlp_gemm_rows_keys_f32(z.data_ptr(), 64, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), rows, 64, 128, z.data_ptr(), z.data_ptr(),
                                         z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), _lib.stream_ptr())
    assert rc != 0 and b"papc_mlp_seg_epi_ok" in lib.papc_last_error_string()
    rng = np.random.default_rng(3)
    Cw = 128
    y = rng.normal(size=(rows, Cw)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, Cw).astype(np.float32) * rng.choice([1.0, -1.0], Cw).astype(np.float32)
    sh = rng.normal(size=Cw).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)
    yd, scd, shd, startd = t(y), t(sc), t(sh), t(lay["start"])
    out = torch.empty(G, Cw, device=dev); am = torch.empty(G, Cw, dtype=torch.int32, device=dev); ys = torch.empty(G, Cw, device=dev)
    _lib.check(lib.papc_bn_relu_max_seg_f32(yd.data_ptr(), Cw, startd.data_ptr(), scd.data_ptr(), shd.data_ptr(), G, out.data_ptr(), am.data_ptr(), ys.data_ptr(),
                                            _lib.stream_ptr()), "seg_max")
    torch.cuda.synchronize()
    want = np.empty((G, Cw), np.int32)
    for g in range(G):
        blk = y[lay["start"][g]:lay["start"][g + 1]] * np.sign(sc)
        want[g] = lay["start"][g] + blk.argmax(0)
    assert np.array_equal(am.cpu().numpy(), want)
    assert np.array_equal(ys.cpu().numpy(), np.take_along_axis(y, want.astype(np.int64), 0))


# ---- the stack: papc_sa_mlp_fwd / _bwd on an SA2-shaped compacted stack ------------------------------------------------------------------------------
B, N, S, D = 2, 128, 32, 128
WIDTHS = [D + 3, 128, 128, 256]


def _lists(dev, radius, seed, scale=1.0):
    x = make_clouds(B, N, seed) * scale
    xyz = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    st = torch.from_numpy(make_start_idx(B, N, seed)).to(dev)
    _, new_xyz = F._fps_raw(xyz, S, st)
    idx = F._ball_query_raw([radius], [K], xyz, new_xyz)[0]
    return xyz.contiguous(), new_xyz.contiguous(), idx.contiguous()


class _Stack:
    """papc_sa_mlp_plan / _fwd called directly, on buffers the test owns (the scratch above all)"""

    def __init__(self, dev, eval_bn=False):
        from papc_amd.mlp import StackSpec
        self.dev = dev
        self.lib = _lib.load()
        ws = seeded_weights(WIDTHS, 61)
        self.params = [torch.from_numpy(a).to(dev) for tup in ws for a in tup]
        self.rm = [(torch.zeros(c, device=dev), torch.ones(c, device=dev)) for c in WIDTHS[1:]]
        self.spec = StackSpec(B, N, S, K, D, True)
        self.spec.eval_bn = eval_bn
        self.cbufs = C.alloc(B * S, K, dev)
        self.xyz = torch.empty(B, N, 3, device=dev)
        self.new_xyz = torch.empty(B, S, 3, device=dev)
        self.idx = torch.empty(B, S, K, dtype=torch.int32, device=dev)
        self.feats = torch.empty(B, N, D, device=dev)

    def load(self, radius, seed, scale=1.0):
        xyz, new_xyz, idx = _lists(self.dev, radius, seed, scale)
        self.xyz.copy_(xyz); self.new_xyz.copy_(new_xyz); self.idx.copy_(idx)
        self.feats.copy_(torch.from_numpy(np.random.default_rng(seed).normal(size=(B, N, D)).astype(np.float32)))
        self.spec.compact = C.plan(self.idx, out=self.cbufs)
        torch.cuda.synchronize()
        return int(self.cbufs[2][0].item())

    def plan(self):
        d = ST.SaDesc()
        d.B, d.N, d.S, d.K, d.D, d.n_layers = B, N, S, K, D, 3
        d.cin = D + 3
        for l in range(3):
            d.cout[l] = WIDTHS[l + 1]
        d.xyz_first, d.pool, d.eval_bn = int(self.spec.xyz_first), 1, int(self.spec.eval_bn)
        d.eps, d.momentum = self.spec.eps, self.spec.momentum
        self.keep = []
        self.io = ST.SaIo()
        ST._fill_io(self.io, self.spec, self.xyz, self.new_xyz, self.feats, self.idx, None, self.params, self.rm, self.keep)
        self.p = ST.SaPlan()
        _lib.check(self.lib.papc_sa_mlp_plan(ctypes.byref(d), ctypes.byref(self.io), ctypes.byref(self.p)), "papc_sa_mlp_plan")
        self.out = torch.empty(B * S, 256, device=self.dev)
        self.saved = torch.zeros(self.p.saved_bytes, dtype=torch.uint8, device=self.dev)
        self.scratch = torch.zeros(self.p.fwd_scratch_bytes, dtype=torch.uint8, device=self.dev)
        self.io.out, self.io.saved, self.io.scratch = self.out.data_ptr(), self.saved.data_ptr(), self.scratch.data_ptr()
        return self.p

    def fwd(self):
        _lib.check(self.lib.papc_sa_mlp_fwd(ctypes.byref(self.p), ctypes.byref(self.io), _lib.stream_ptr()), "papc_sa_mlp_fwd")

    def result(self, rows):
        """(out, argmax, the last layer's stored y on the physical rows) -- copies"""
        torch.cuda.synchronize()
        am = self.saved[self.p.off_argmax:self.p.off_argmax + 4 * B * S * 256].view(torch.int32).clone()
        y = self.saved[self.p.off_y[2]:self.p.off_y[2] + 4 * rows * 256].view(torch.int32).clone()
        return self.out.clone().view(torch.int32), am, y


def test_scratch_contents_and_graph_replay_do_not_matter(dev):
    """the key buffer lives in the caller's scratch and is cleared inside the call: the same call on scratch full of 0xFF bytes, and a captured
    call replayed on another batch (another device-side row count, other groups), equal a fresh run bit for bit"""
    s = _Stack(dev)
    rows_a = s.load(0.6, 31)
    p = s.plan()
    assert p.compact == 1 and s.lib.papc_mlp_seg_epi_ok(B * S * K, 128, 256) == 1
    with _seg_epi(1):
        s.fwd()
        fresh_a = s.result(rows_a)
        s.scratch.fill_(0xFF)
        s.fwd()
        again = s.result(rows_a)
        for u, v in zip(again, fresh_a):
            assert torch.equal(u, v), "the result depends on what the scratch held"
        # ---- captured, replayed on batch a and then on batch b
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                s.fwd()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        s.scratch.fill_(0xFF)
        g.replay()
        rep_a = s.result(rows_a)
        for u, v in zip(rep_a, fresh_a):
            assert torch.equal(u, v), "graph replay differs from the eager call"
        rows_b = s.load(0.45, 32, 0.8)
        assert rows_b != rows_a
        g.replay()
        rep_b = s.result(rows_b)
        f = _Stack(dev)
        assert f.load(0.45, 32, 0.8) == rows_b
        f.plan()
        f.fwd()
        fresh_b = f.result(rows_b)
    with _seg_epi(0):
        f.fwd()
        parent_b = f.result(rows_b)
    for u, v, w_ in zip(rep_b, fresh_b, parent_b):
        assert torch.equal(u, v), "replay on another batch differs from a fresh run"
        assert torch.equal(v, w_), "PAPC_SEG_EPI=1 differs from PAPC_SEG_EPI=0"


def _stack_fwd_bwd(dev, knob, seed, train=True):
    from papc_amd.mlp import StackSpec, shared_mlp_max
    from papc_amd.stack import SharedMLPStack
    xyz, new_xyz, idx = _lists(dev, 0.6, seed)
    feats = torch.from_numpy(np.random.default_rng(seed).normal(size=(B, N, D)).astype(np.float32)).to(dev).requires_grad_(True)
    ws = seeded_weights(WIDTHS, 50 + seed)
    params = [torch.from_numpy(a).to(dev).requires_grad_(True) for tup in ws for a in tup]
    spec = StackSpec(B, N, S, K, D, True)
    bn = None
    if not train:
        spec.eval_bn = True
        bn = [(torch.from_numpy(np.random.default_rng(l).normal(size=c).astype(np.float32) * 0.1).to(dev),
               torch.from_numpy(np.random.default_rng(l).uniform(0.5, 1.5, c).astype(np.float32)).to(dev)) for l, c in enumerate(WIDTHS[1:])]
    spec.compact = C.plan(idx)
    if train:      # the grouping's point lists, as a training layer makes them: the gather-add backward is then a sum in fixed order (no float atomics)
        spec.plists = C.point_lists(xyz, new_xyz, idx, spec.compact)
    with _seg_epi(knob):
        out = shared_mlp_max(spec, bn, xyz, new_xyz, feats, idx, params)
        node = out.grad_fn
        am = SharedMLPStack.views(node)[0].clone() if type(node).__name__.startswith("SharedMLPStack") else None
        if train:
            gout = torch.from_numpy(np.random.default_rng(7).normal(size=tuple(out.shape)).astype(np.float32)).to(dev)
            out.backward(gout)
    torch.cuda.synchronize()
    return spec, node, out.detach(), am, [p.grad.clone() for p in params] if train else None, feats.grad.clone() if train else None


def test_stack_is_bit_identical_with_and_without_the_epilogue(dev):
    """an SA2-shaped compacted stack (131 -> 128 -> 128 -> 256, B = 2, 128 points, 32 centroids, nsample 64), forward and backward:
    PAPC_SEG_EPI=1 against 0 -- output, argmax, every parameter gradient and the input gradient as integers"""
    res = {}
    for knob in (0, 1):
        spec, node, out, am, grads, gf = _stack_fwd_bwd(dev, knob, 4)
        assert node.compact is not None, "the compacted path was not taken"
        res[knob] = (out, am, grads, gf)
    frac = spec.compact.fraction()
    print("physical rows / padded rows: %.3f" % frac)
    assert 0.3 < frac < 0.75, "the radius should leave about half the slots as copies"
    (o0, a0, g0, f0), (o1, a1, g1, f1) = res[0], res[1]
    assert a0 is not None and torch.equal(a1, a0), "argmax differs"
    assert torch.equal(_bits(o1), _bits(o0)), "output differs"
    for i, (u, v) in enumerate(zip(g1, g0)):
        assert torch.equal(_bits(u), _bits(v)), "gradient of parameter %d differs" % i
    assert torch.equal(_bits(f1), _bits(f0)), "input gradient differs"
    assert float(o1.abs().max()) > 0 and float(f1.abs().max()) > 0


def test_eval_mode_keeps_its_path(dev):
    """eval-mode BatchNorm is never compacted and never takes the epilogue: the knob changes nothing there"""
    r0 = _stack_fwd_bwd(dev, 0, 4, train=False)
    r1 = _stack_fwd_bwd(dev, 1, 4, train=False)
    assert r1[1].compact is None
    assert torch.equal(_bits(r1[2]), _bits(r0[2])) and torch.equal(r1[3], r0[3])
    assert torch.isfinite(r1[2]).all() and float(r1[2].abs().max()) > 0
