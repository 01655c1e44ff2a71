"""The 3x3 conv2d product loops (csrc/conv2d.hip: forward, dX, dW) held to the EXACT fp32 product, bit for bit: a sibling of
tests/test_gpu_exact_loaders.py on the probe pool of tests/test_gpu_exact_products.py (that file's docstring has the method: three-plane probe
pairs, single terms and 2 / 4 equal terms, the int32 comparison, no tolerance).

  papc_conv2d_fwd_f32      the input zero but for a period-3 lattice of pixels per axis, ONE positive channel per lattice pixel: a 3-wide window
                           holds at most one lattice pixel under stride 1 and stride 2 alike, so every output element is one term
                           x[pixel, ci] W[co, ci, tap] or an exact zero; run on plain rows and through the norm-on-load flavour with scale 1, shift 0
  papc_conv2d_bwd_dx_f32   dz non-zero in ONE channel of the output pixels on a period-3 (stride 2: period-2) lattice: an input pixel meets at most one of them through
                           one tap -- under stride 2 only through the taps of matching parity -- so dX is one term dz W[co, ci, tap] or an exact
                           zero; mean 0, 1/sigma 1, scale 1, c1 = c2 = 0 make dY = dz; no addend, no norm above
  papc_conv2d_bwd_dw_f32   the input dense and identical in each of four frames, channel co has its gradient at one output pixel in 4, 2 or 1
                           frames: Cout Cin 9 sums of 4, 2, 1 equal terms (an exact zero where the tap falls into the halo), folded over the chunks

test_every_conv2d_case (NumPy, runs everywhere) verifies every operand set with Probe.verify() and asserts that taps, both strides' parities,
channels and planes are covered.
"""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib
from tests.test_gpu_exact_products import F32, F64, POOL, Probe, Tally, _scale_b, _sign, dev_, full, gpu

NAN = float("nan")
CLOUDS = ((0, 1, 2, 3), (1, 3), (2,))                    # the frames (of four) in which class s of the dW cases has its gradient
FWD_SHAPES = ((2, 11, 13, 64, 64, 1), (2, 11, 13, 32, 64, 2))      # (B, H, W, Cin, Cout, stride): two row tiles, a ragged last one
DW_SHAPE = (4, 12, 14)                                   # 672 output rows under stride 1: three chunks of 256; 168 under stride 2: one ragged chunk


def _fl32(x):
    return np.asarray(x, F64).astype(F32).astype(F64)


def out_edge(n, s):
    return (n - 1) // s + 1


def _im2col(x, s):
    """x [B, H, W, C] -> [B Ho Wo, 9 C] with the zero halo, tap-major K (k = tap C + c, tap = 3 ty + tx)"""
    B, H, W, C = x.shape
    Ho, Wo = out_edge(H, s), out_edge(W, s)
    xp = np.zeros((B, H + 2, W + 2, C), F64)
    xp[:, 1:-1, 1:-1] = x
    cols = np.zeros((B, Ho, Wo, 9 * C), F64)
    for t in range(9):
        ty, tx = t // 3, t % 3
        cols[..., C * t:C * t + C] = xp[:, ty:ty + s * (Ho - 1) + 1:s, tx:tx + s * (Wo - 1) + 1:s]
    return cols.reshape(B * Ho * Wo, 9 * C)


# ---- forward --------------------------------------------------------------------------------------------------------------------------
def fwd_operands(shape):
    """im2col form: A [B Ho Wo, 9 Cin], B = wk [Cout, 9 Cin]; expect = y.  The pair is a function of ci"""
    Bn, H, W, Cin, Cout, s = shape
    ids = POOL.pairs(1)
    pk = ids[np.arange(Cin) % ids.size]
    x = np.zeros((Bn, H, W, Cin), F64)
    lat = 0
    for b in range(Bn):
        for h in range(b % 3, H, 3):
            for w in range((b + 1) % 3, W, 3):
                ci = (7 * lat + 3) % Cin
                x[b, h, w, ci] = float(POOL.a[pk[ci]]) * 2.0 ** (((h + 2 * w) % 7) - 3)
                lat += 1
    A = _im2col(x, s)
    assert ((A != 0).sum(axis=1) <= 1).all(), "a 3-wide window holds at most one lattice pixel"
    co, k = np.meshgrid(np.arange(Cout), np.arange(9 * Cin), indexing="ij")
    Bm = POOL.b[pk[k % Cin]].astype(F64) * _scale_b(co, k) * _sign(co, k)
    kk = np.nonzero(A)[1]
    pr = Probe(A, Bm, _fl32(A @ Bm.T), {int(p): 1 for p in set(pk[kk % Cin])})
    pr.taps, pr.cis, pr.live = np.unique(kk // Cin), np.unique(kk % Cin), float((A != 0).any(axis=1).mean())
    pr.x = x.reshape(-1, Cin).astype(F32)
    pr.w = np.ascontiguousarray(Bm.reshape(Cout, 9, Cin).transpose(0, 2, 1)).astype(F32)          # [co][tap][ci] -> [co][ci][tap]
    return pr


# ---- dX ---------------------------------------------------------------------------------------------------------------------------------
def dx_operands(shape):
    """A [B H W, 9 Cout] (k = tap Cout + co): the dY an input pixel meets through tap; B = wt [Cin, 9 Cout]; expect = dX.  The pair is a function
    of co"""
    Bn, H, W, Cin, Cout, s = shape
    Ho, Wo = out_edge(H, s), out_edge(W, s)
    ids = POOL.pairs(1)
    pk = ids[np.arange(Cout) % ids.size]
    dz = np.zeros((Bn, Ho, Wo, Cout), F64)
    A = np.zeros((Bn, H, W, 9 * Cout), F64)
    live, cos, par = 0, [], set()
    per = 3 if s == 1 else 2                                 # under stride 2 an input pixel sees at most two adjacent output pixels per axis
    for b in range(Bn):
        for qh in range(b % per, Ho, per):
            for qw in range((b + 2) % per, Wo, per):
                co = (5 * live + 1) % Cout
                v = float(POOL.a[pk[co]]) * 2.0 ** ((live % 7) - 3) * (-1.0 if live % 3 == 0 else 1.0)
                dz[b, qh, qw, co] = v
                for t in range(9):
                    ph, pw = s * qh + t // 3 - 1, s * qw + t % 3 - 1                               # the input pixel output (qh, qw) reads through tap t
                    if 0 <= ph < H and 0 <= pw < W:
                        A[b, ph, pw, Cout * t + co] = v
                        par.add((ph % 2, pw % 2, t))
                cos.append(co)
                live += 1
    A = A.reshape(Bn * H * W, 9 * Cout)
    assert ((A != 0).sum(axis=1) <= 1).all(), "an input pixel meets at most one live output pixel"
    ci, k = np.meshgrid(np.arange(Cin), np.arange(9 * Cout), indexing="ij")
    Bm = POOL.b[pk[k % Cout]].astype(F64) * _scale_b(ci, k) * _sign(ci, k)
    pr = Probe(A, Bm, _fl32(A @ Bm.T), {int(p): 1 for p in set(pk[cos])})
    pr.taps, pr.cos, pr.par, pr.live = np.unique(np.nonzero(A)[1] // Cout), set(cos), par, float((A != 0).any(axis=1).mean())
    pr.dz = dz.reshape(-1, Cout).astype(F32)
    pr.w = np.ascontiguousarray(Bm.reshape(Cin, 9, Cout).transpose(2, 0, 1)).astype(F32)          # [ci][tap][co] -> [co][ci][tap]
    return pr


# ---- dW ---------------------------------------------------------------------------------------------------------------------------------
def dw_operands(which, s, Cin=32, Cout=64):
    """A = dz^T [Cout, B Ho Wo], B [9 Cin (tap Cin + ci), B Ho Wo] = the input under tap of that row's window; expect [co][tap][ci].  One pair per case"""
    Bn, H, W = DW_SHAPE
    Ho, Wo = out_edge(H, s), out_edge(W, s)
    mo = Ho * Wo
    p = int(POOL.pairs(4)[which])
    i, c = np.meshgrid(np.arange(H * W), np.arange(Cin), indexing="ij")
    xc = (float(POOL.b[p]) * 2.0 ** (((5 * i + 2 * c) % 9) - 4) * np.where((i + c) % 3 == 0, -1.0, 1.0)).reshape(1, H, W, Cin)
    co = np.arange(Cout)
    cls, row = co % 3, (41 * co + 7) % mo
    dv = float(POOL.a[p]) * 2.0 ** ((co % 7) - 3) * _sign(co, 1)
    dz = np.zeros((Bn * mo, Cout), F64)
    for c_ in co:
        for b in CLOUDS[cls[c_]]:
            dz[b * mo + row[c_], c_] = dv[c_]
    Bm = np.tile(_im2col(xc, s).T.reshape(9 * Cin, 1, mo), (1, Bn, 1)).reshape(9 * Cin, Bn * mo)
    pr = Probe(dz.T, Bm, _fl32(dz.T @ Bm.T), {p: 4})
    pr.dz, pr.x = dz.astype(F32), np.tile(xc.reshape(1, -1, Cin), (Bn, 1, 1)).reshape(-1, Cin).astype(F32)
    pr.dw = np.ascontiguousarray(pr.expect.reshape(Cout, 9, Cin).transpose(0, 2, 1))              # the source's [co][ci][tap]
    rpc = max(256, -(-(-(-Bn * mo // 64)) // 16) * 16)                                            # conv2d.hip: c2d_dw_rpc
    pr.chunks = sorted({int(b * mo + row[c_]) // rpc for c_ in co for b in CLOUDS[cls[c_]]})
    pr.nchunks = -(-Bn * mo // rpc)
    pr.halo = float((pr.expect == 0).mean())
    return pr


def _all_probes():
    for shape in FWD_SHAPES:
        yield "conv2d forward %s" % (shape,), fwd_operands(shape)
        yield "conv2d dX %s" % (shape,), dx_operands(shape)
    for which in (0, 2):
        for s in (1, 2):
            yield "conv2d dW, pair %d stride %d" % (which, s), dw_operands(which, s)


def test_every_conv2d_case():
    """every operand set through Probe.verify(), and the coverage the cases lean on: all nine taps, both parities of an input pixel under
    stride 2 on both axes, channels in both halves of a k step and beyond the first 32-column block, sums of 4, 2 and 1 terms over all chunks"""
    assert POOL.pairs(4).size >= 3
    n = 0
    for name, pr in _all_probes():
        pr.verify()
        n += 1
    for shape in FWD_SHAPES:
        Cin, Cout, s = shape[3], shape[4], shape[5]
        pr = fwd_operands(shape)
        print("[conv2d exact] forward %s: %.2f of the rows live, %d ci" % (shape, pr.live, pr.cis.size))
        assert pr.taps.size == 9 and pr.live >= 0.5 and pr.cis.size >= min(Cin, 24)
        assert all(((pr.cis % 16) // 8 == h_).any() for h_ in (0, 1)) and (pr.cis >= Cin // 2).any()
        pr = dx_operands(shape)
        print("[conv2d exact] dX %s: %.2f of the rows live, %d co" % (shape, pr.live, len(pr.cos)))
        assert pr.taps.size == 9 and pr.live >= 0.2 and len(pr.cos) >= 16 and any(c >= 32 for c in pr.cos)
        assert all(any((c % 16) // 8 == h_ for c in pr.cos) for h_ in (0, 1))
        if s == 2:            # a tap reaches only the input pixels of its parity: (ph + 1 - ty) even, on both axes, and every such combination occurs
            assert all((ph + 1 - t // 3) % 2 == 0 and (pw + 1 - t % 3) % 2 == 0 for ph, pw, t in pr.par)
            assert {(ph, pw) for ph, pw, _ in pr.par} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {t for _, _, t in pr.par} == set(range(9))
    for which in (0, 2):
        for s in (1, 2):
            pr = dw_operands(which, s)
            assert pr.chunks == list(range(pr.nchunks)) and pr.nchunks == (3 if s == 1 else 1), "gradient rows in every chunk"
            assert 0 < pr.halo < 0.2 and (pr.dw != 0).any(axis=(0, 1)).all(), "a few taps fall into the halo, every tap carries terms"
            assert sorted(set((pr.dz != 0).sum(axis=0).tolist())) == [1, 2, 4], "classes of 4, 2 and 1 equal terms"
    print("[conv2d exact] %d case operand sets verified" % n)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
def run_prep(dev, w, Cin, Cout):
    """papc_conv2d_prep_f32: wk = W[co][tap][ci], wt = W[ci][tap][co], compared with the NumPy transposes bit for bit"""
    wd, wk, wt = dev_(w, dev), full((Cout, 9, Cin), NAN, dev), full((Cin, 9, Cout), NAN, dev)
    one_p, one_i = ctypes.c_void_p * 1, ctypes.c_int * 1
    _lib.check(_lib.load().papc_conv2d_prep_f32(one_p(wd.data_ptr()), one_p(wk.data_ptr()), one_p(wt.data_ptr()), one_i(Cin), one_i(Cout), one_i(1), one_i(0), 1,
                                                _lib.stream_ptr()), "papc_conv2d_prep_f32")
    assert np.array_equal(wk.cpu().numpy().view(np.int32), np.ascontiguousarray(w.transpose(0, 2, 1)).view(np.int32)) and \
        np.array_equal(wt.cpu().numpy().view(np.int32), np.ascontiguousarray(w.transpose(1, 2, 0)).view(np.int32)), "wk / wt are not the transposes of w"
    return wk, wt


@gpu
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv2d_forward(dev, shape):
    """c2d_fwd_kernel, both flavours: plain rows, and scale 1, shift 0 on the positive lattice values"""
    lib = _lib.load()
    Bn, H, W, Cin, Cout, s = shape
    pr = fwd_operands(shape)
    tally = Tally("conv2d forward %s" % (shape,))
    wk, _ = run_prep(dev, pr.w, Cin, Cout)
    x, sc, sh = dev_(pr.x, dev), torch.ones(Cin, device=dev), torch.zeros(Cin, device=dev)
    Mo = Bn * out_edge(H, s) * out_edge(W, s)
    for scp, shp, what in ((0, 0, "y, plain rows"), (sc.data_ptr(), sh.data_ptr(), "y, norm on load")):
        y, part = full((Mo, Cout), NAN, dev), torch.empty(lib.papc_conv2d_parts(Mo), 2, Cout, device=dev)
        _lib.check(lib.papc_conv2d_fwd_f32(x.data_ptr(), scp, shp, wk.data_ptr(), Bn, H, W, Cin, Cout, s, y.data_ptr(), part.data_ptr(), _lib.stream_ptr()),
                   "papc_conv2d_fwd_f32")
        tally.add(y, pr.expect, what)
    tally.done()


@gpu
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv2d_bwd_dx(dev, shape):
    """c2d_dx_kernel: mean 0, 1/sigma 1, scale 1, c1 = c2 = 0 (dY = dz), y = 0, no addend, no norm above"""
    lib = _lib.load()
    Bn, H, W, Cin, Cout, s = shape
    pr = dx_operands(shape)
    tally = Tally("conv2d dX %s" % (shape,))
    _, wt = run_prep(dev, pr.w, Cin, Cout)
    dz, y = dev_(pr.dz, dev), torch.zeros(pr.dz.shape, device=dev)
    zero, one = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
    dx = full((Bn * H * W, Cin), NAN, dev)
    _lib.check(lib.papc_conv2d_bwd_dx_f32(dz.data_ptr(), y.data_ptr(), zero.data_ptr(), one.data_ptr(), one.data_ptr(), zero.data_ptr(), zero.data_ptr(),
                                          wt.data_ptr(), Bn, H, W, Cin, Cout, s, 0, 0, 0, 0, 0, 0, dx.data_ptr(), 0, _lib.stream_ptr()), "papc_conv2d_bwd_dx_f32")
    tally.add(dx, pr.expect, "dX")
    tally.done()


@gpu
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("which", [0, 2])
def test_conv2d_bwd_dw(dev, which, s):
    """c2d_dw_kernel and its chunk fold: y = 0, mean 0, 1/sigma 1, scale 1, c1 = c2 = 0, plain input rows; sums of 4, 2, 1 equal terms"""
    lib = _lib.load()
    Bn, H, W = DW_SHAPE
    Cin, Cout = 32, 64
    pr = dw_operands(which, s)
    tally = Tally("conv2d dW, pair %d stride %d" % (which, s))
    dz, x, y = dev_(pr.dz, dev), dev_(pr.x, dev), torch.zeros(pr.dz.shape, device=dev)
    zero, one = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
    nb = lib.papc_conv2d_bwd_dw_workspace(Bn, H, W, Cin, Cout, s)
    assert nb == pr.nchunks * Cout * Cin * 9 * 4
    ws, dw = full((nb // 4,), NAN, dev), full((Cout, Cin, 9), NAN, dev)
    _lib.check(lib.papc_conv2d_bwd_dw_f32(dz.data_ptr(), y.data_ptr(), zero.data_ptr(), one.data_ptr(), one.data_ptr(), zero.data_ptr(), zero.data_ptr(),
                                          x.data_ptr(), 0, 0, Bn, H, W, Cin, Cout, s, dw.data_ptr(), 0, ws.data_ptr(), nb, _lib.stream_ptr()),
               "papc_conv2d_bwd_dw_f32")
    tally.add(dw, pr.dw, "dW")
    tally.done()
