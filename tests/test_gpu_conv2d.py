"""GPU tests of csrc/conv2d.hip through the C ABI: the 3x3 family (stride 1 and 2, zero halo) and the kernel = stride deconvolutions, forward,
dX (with and without the addend, with and without a norm above) and dW, against float64 (F.conv2d / F.conv_transpose2d on the CPU).  Outputs
are pre-filled with NaN, workspaces with 0xA5; inputs are randn; the producer's shift is positive in about half the channels, so that a halo
filled with relu(shift) instead of the exact 0 lands on wrong values.  Backward comparisons are routed by the kernels' own ReLU signs."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from papc_amd import _lib
from tests.util import assert_close

pytestmark = pytest.mark.gpu
BAR = 2e-4          # the project's model-level bar (as tests/test_gpu_voxnet.py, tests/test_gpu_kdnet.py)
EPS, MOM = 1e-3, 0.01
POISON = 777.0

CONV_CASES = [(1, 5, 7, 32, 32, 1),          # below one tile, odd
              (2, 9, 13, 64, 64, 2),         # odd extent under stride 2 -> 5 x 7, right/bottom parity
              (2, 16, 24, 64, 128, 2),       # a KITTI width pair
              (1, 8, 12, 128, 256, 2),       # a KITTI width pair
              (3, 6, 10, 256, 256, 1),       # a KITTI width pair
              (1, 33, 40, 64, 64, 1)]        # several spatial tiles, ragged last tile on both axes
DECONV_CASES = [(2, 3, 5, 64, 128, 1), (1, 6, 4, 128, 128, 2), (2, 2, 3, 256, 128, 4)]


def _np(t):
    return t.detach().double().cpu().numpy()


def _nan(*shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _rows(t):
    """NCHW -> channel-last rows"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw(rows, B, H, W):
    return rows.view(B, H, W, -1).permute(0, 3, 1, 2)


def _c12p(c12):
    return c12[0].data_ptr(), c12[1].data_ptr()


class _Case:
    """the inputs of one layer (fp32 values, kept in float64 for the reference and in fp32 on the device)"""

    def __init__(self, dev, deconv, B, H, W, Cin, Cout, s, norm, seed):
        g = torch.Generator().manual_seed(seed)
        rn = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64).float()               # noqa: E731
        ru = lambda *sh: (0.5 + torch.rand(*sh, generator=g, dtype=torch.float64)).float()        # noqa: E731
        self.dev, self.deconv, self.norm, self.dims = dev, deconv, norm, (B, H, W, Cin, Cout, s)
        self.Ho, self.Wo = (s * H, s * W) if deconv else ((H - 1) // s + 1, (W - 1) // s + 1)
        self.Mi, self.Mo = B * H * W, B * self.Ho * self.Wo
        self.ld, self.coff = (Cout + 64, 32) if deconv else (Cout, 0)
        self.x = rn(self.Mi, Cin)
        self.mean_p, self.invstd_p = 0.2 * rn(Cin), ru(Cin)
        gamma_p = ru(Cin)
        gamma_p[1] = -gamma_p[1]
        self.sc_in = gamma_p * self.invstd_p
        self.sh_in = 0.5 * rn(Cin) - self.mean_p * self.sc_in
        assert 0.25 < float((self.sh_in > 0).float().mean()) < 0.75                                # a halo of relu(shift) would be non-zero in about half the channels
        self.w = rn(Cin, Cout, s, s) / Cin ** 0.5 if deconv else rn(Cout, Cin, 3, 3) / (9 * Cin) ** 0.5
        self.gamma, self.beta = ru(Cout), 0.3 * rn(Cout)
        self.gamma[2] = -self.gamma[2]
        self.gout = rn(self.Mo, self.ld)
        self.addend = rn(self.Mi, Cin)
        self.d = {k: getattr(self, k).to(dev) for k in ("x", "mean_p", "invstd_p", "sc_in", "sh_in", "w", "gamma", "beta", "gout", "addend")}

    # ---- float64 ----
    def ref_forward(self, sign_prev=None, sign=None, grad=False):
        B, H, W, Cin, Cout, s = self.dims
        v = lambda t: t.double().view(1, -1, 1, 1)                                                # noqa: E731
        L = {"x": _nchw(self.x.double(), B, H, W).clone().requires_grad_(grad), "w": self.w.double().clone().requires_grad_(grad),
             "gamma": self.gamma.double().clone().requires_grad_(grad), "beta": self.beta.double().clone().requires_grad_(grad)}
        a = L["x"]
        if self.norm:
            tp = v(self.sc_in) * L["x"] + v(self.sh_in)
            if grad:
                tp.retain_grad()
            sp = (tp.detach() > 0) if sign_prev is None else sign_prev
            a = torch.where(sp, tp, torch.zeros_like(tp))
            L["tp"], L["sp"] = tp, sp
        y = F.conv_transpose2d(a, L["w"], None, stride=s) if self.deconv else F.conv2d(F.pad(a, (1, 1, 1, 1)), L["w"], None, stride=s)
        mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
        t = (y - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + EPS) * L["gamma"].view(1, -1, 1, 1) + L["beta"].view(1, -1, 1, 1)
        if grad:
            t.retain_grad()
        sg = (t.detach() > 0) if sign is None else sign
        L.update(y=y, mean=mean, var=var, t=t, out=torch.where(sg, t, torch.zeros_like(t)))
        return L

    # ---- the kernels ----
    def kernel_forward(self, lib):
        B, H, W, Cin, Cout, s = self.dims
        dev, st, d = self.dev, _lib.stream_ptr(), self.d
        n = self.w.numel()
        wk, wt = _nan(n, dev=dev), _nan(n, dev=dev)
        one_p, one_i = ctypes.c_void_p * 1, ctypes.c_int * 1
        _lib.check(lib.papc_conv2d_prep_f32(one_p(d["w"].data_ptr()), one_p(wk.data_ptr()), one_p(wt.data_ptr()), one_i(Cin), one_i(Cout), one_i(s),
                                            one_i(int(self.deconv)), 1, st), "prep")
        y = torch.full((self.Mo, self.ld), POISON, device=dev)
        y[:, self.coff:self.coff + Cout] = float("nan")
        sc, sh = (d["sc_in"].data_ptr(), d["sh_in"].data_ptr()) if self.norm else (0, 0)
        if self.deconv:
            parts = lib.papc_conv2d_parts(self.Mi) * s * s
            part = _nan(parts, 2, Cout, dev=dev)
            _lib.check(lib.papc_deconv2d_fwd_f32(d["x"].data_ptr(), sc, sh, wk.data_ptr(), B, H, W, Cin, Cout, s, y.data_ptr(), self.ld, self.coff,
                                                 part.data_ptr(), st), "deconv fwd")
        else:
            parts = lib.papc_conv2d_parts(self.Mo)
            assert parts == -(-self.Mo // 128)
            part = _nan(parts, 2, Cout, dev=dev)
            _lib.check(lib.papc_conv2d_fwd_f32(d["x"].data_ptr(), sc, sh, wk.data_ptr(), B, H, W, Cin, Cout, s, y.data_ptr(), part.data_ptr(), st), "conv fwd")
        cst, rmean, rvar = _nan(4, Cout, dev=dev), torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
        _lib.check(lib.papc_bn_finalize_f32(part.data_ptr(), parts, self.Mo, Cout, d["gamma"].data_ptr(), d["beta"].data_ptr(), EPS, MOM, *_lib.cst_ptrs(cst),
                                            rmean.data_ptr(), rvar.data_ptr(), st), "finalize")
        return {"wk": wk, "wt": wt, "y": y, "part": part, "cst": cst, "rmean": rmean, "rvar": rvar}

    def kernel_backward(self, lib, f):
        B, H, W, Cin, Cout, s = self.dims
        dev, st, d = self.dev, _lib.stream_ptr(), self.d
        mean, invstd, scale, shift = _lib.cst_ptrs(f["cst"])
        res = {"dz": torch.full((self.Mo, self.ld), POISON, device=dev), "dgamma": _nan(Cout, dev=dev), "dbeta": _nan(Cout, dev=dev), "c12": _nan(2, Cout, dev=dev)}
        res["dz"][:, self.coff:self.coff + Cout] = float("nan")
        rparts = lib.papc_conv2d_relu_bwd_parts(self.Mo)
        red = _nan(rparts, 2, Cout, dev=dev)
        _lib.check(lib.papc_conv2d_relu_bwd_f32(d["gout"].data_ptr(), f["y"].data_ptr(), self.ld, self.coff, mean, invstd, scale, shift, self.Mo, Cout,
                                                res["dz"].data_ptr(), red.data_ptr(), st), "relu bwd")
        _lib.check(lib.papc_bn_bwd_finalize_f32(red.data_ptr(), rparts, self.Mo, Cout, res["dgamma"].data_ptr(), res["dbeta"].data_ptr(), *_c12p(res["c12"]), 0, st),
                   "bwd finalize")
        pparts = lib.papc_conv2d_parts(self.Mi)
        prev = (d["x"].data_ptr(), d["mean_p"].data_ptr(), d["invstd_p"].data_ptr(), d["sc_in"].data_ptr(), d["sh_in"].data_ptr()) if self.norm else (0,) * 5
        for tag, add in (("", 0), ("_add", d["addend"].data_ptr())):
            dx, redp = _nan(self.Mi, Cin, dev=dev), _nan(pparts, 2, Cin, dev=dev)
            if self.deconv:
                _lib.check(lib.papc_deconv2d_bwd_dx_f32(res["dz"].data_ptr(), f["y"].data_ptr(), self.ld, self.coff, mean, invstd, scale, *_c12p(res["c12"]),
                                                        f["wt"].data_ptr(), B, H, W, Cin, Cout, s, add, *prev, dx.data_ptr(), redp.data_ptr() if self.norm else 0,
                                                        st), "deconv dx")
            else:
                _lib.check(lib.papc_conv2d_bwd_dx_f32(res["dz"].data_ptr(), f["y"].data_ptr(), mean, invstd, scale, *_c12p(res["c12"]), f["wt"].data_ptr(), B, H, W,
                                                      Cin, Cout, s, add, *prev, dx.data_ptr(), redp.data_ptr() if self.norm else 0, st), "conv dx")
            res["dx" + tag] = dx
            if self.norm:
                res["redp" + tag] = redp
                sums, c12p = _nan(2, Cin, dev=dev), _nan(2, Cin, dev=dev)
                _lib.check(lib.papc_bn_bwd_finalize_f32(redp.data_ptr(), pparts, self.Mi, Cin, sums[0].data_ptr(), sums[1].data_ptr(), *_c12p(c12p), 0, st),
                           "bwd finalize prev")
                res["sums" + tag] = sums                                                          # (sum dz xhat, sum dz) = (dgamma, dbeta) of the producer
        sc, sh = (d["sc_in"].data_ptr(), d["sh_in"].data_ptr()) if self.norm else (0, 0)
        wsf = lib.papc_deconv2d_bwd_dw_workspace if self.deconv else lib.papc_conv2d_bwd_dw_workspace
        nb = wsf(B, H, W, Cin, Cout, s)
        assert nb > 0 and nb % 16 == 0
        for tag, acc in (("", 0), ("_acc", 1)):
            ws = torch.full((nb,), 0xA5, device=dev, dtype=torch.uint8)
            dw = _nan(*self.w.shape, dev=dev) if not acc else torch.ones(*self.w.shape, device=dev)
            if self.deconv:
                _lib.check(lib.papc_deconv2d_bwd_dw_f32(res["dz"].data_ptr(), f["y"].data_ptr(), self.ld, self.coff, mean, invstd, scale, *_c12p(res["c12"]),
                                                        d["x"].data_ptr(), sc, sh, B, H, W, Cin, Cout, s, dw.data_ptr(), acc, ws.data_ptr(), nb, st), "deconv dw")
            else:
                _lib.check(lib.papc_conv2d_bwd_dw_f32(res["dz"].data_ptr(), f["y"].data_ptr(), mean, invstd, scale, *_c12p(res["c12"]), d["x"].data_ptr(), sc, sh,
                                                      B, H, W, Cin, Cout, s, dw.data_ptr(), acc, ws.data_ptr(), nb, st), "conv dw")
            res["dw" + tag] = dw
        return res


def _check(dev, deconv, case, norm, seed):
    lib = _lib.load()
    B, H, W, Cin, Cout, s = case
    tag = "%s %s %s" % ("deconv" if deconv else "conv", case, "norm-on-load" if norm else "plain")
    c = _Case(dev, deconv, B, H, W, Cin, Cout, s, norm, seed)
    f = c.kernel_forward(lib)
    cols = slice(c.coff, c.coff + Cout)
    # ---- forward against the reference's own decisions
    ref = c.ref_forward()
    yk = f["y"][:, cols]
    assert bool(torch.isfinite(yk).all()), "unwritten output " + tag
    assert_close(_np(yk), _np(_rows(ref["y"])), BAR, "y " + tag)
    assert_close(_np(f["cst"][0]), _np(ref["mean"]), BAR, "mean " + tag)
    assert_close(_np(f["cst"][1]), _np(1.0 / torch.sqrt(ref["var"] + EPS)), BAR, "1/sigma " + tag)
    assert_close(_np(f["rmean"]), _np((1.0 - MOM) * ref["mean"]), BAR, "running mean " + tag)      # 0.01 * 0 + 0.99 * batch
    assert_close(_np(f["rvar"]), _np(MOM + (1.0 - MOM) * ref["var"]), BAR, "running var (biased) " + tag)
    if deconv:                                                                                    # the neighbouring columns of the concat buffer
        assert bool((f["y"][:, :c.coff] == POISON).all()) and bool((f["y"][:, c.coff + Cout:] == POISON).all()), "neighbouring columns written " + tag
    # ---- backward against float64 routed by the kernels' own signs
    res = c.kernel_backward(lib, f)
    sign = _nchw(((f["cst"][2].double() * yk.double() + f["cst"][3].double()) > 0).cpu(), B, c.Ho, c.Wo)
    sign_prev = _nchw(((c.sc_in.double() * c.x.double() + c.sh_in.double()) > 0), B, H, W) if norm else None
    pin = c.ref_forward(sign_prev, sign, grad=True)
    (pin["out"] * _nchw(c.gout[:, cols].double(), B, c.Ho, c.Wo)).sum().backward()
    assert_close(_np(res["dz"][:, cols]), _np(_rows(pin["t"].grad)), BAR, "dz " + tag)
    assert bool((res["dz"][:, :c.coff] == POISON).all()) and bool((res["dz"][:, c.coff + Cout:] == POISON).all()), "neighbouring dz columns written " + tag
    assert_close(_np(res["dgamma"]), _np(pin["gamma"].grad), BAR, "dgamma " + tag)
    assert_close(_np(res["dbeta"]), _np(pin["beta"].grad), BAR, "dbeta " + tag)
    add = c.addend.double()
    if norm:
        dzp = _rows(pin["tp"].grad)
        sp = _rows(sign_prev)
        xhat = (c.x.double() - c.mean_p.double()) * c.invstd_p.double()
        for t_, want in (("", dzp), ("_add", dzp + torch.where(sp, add, torch.zeros_like(add)))):
            assert_close(_np(res["dx" + t_]), _np(want), BAR, "dz_prev%s %s" % (t_, tag))
            assert_close(_np(res["sums" + t_][1]), _np(want.sum(0)), BAR, "sum dz_prev%s %s" % (t_, tag))
            assert_close(_np(res["sums" + t_][0]), _np((want * xhat).sum(0)), BAR, "sum dz_prev xhat%s %s" % (t_, tag))
    else:
        dx = _rows(pin["x"].grad)
        assert_close(_np(res["dx"]), _np(dx), BAR, "dx " + tag)
        assert_close(_np(res["dx_add"]), _np(dx + add), BAR, "dx + addend " + tag)
    assert_close(_np(res["dw"]), _np(pin["w"].grad), BAR, "dw " + tag)
    assert_close(_np(res["dw_acc"]), _np(pin["w"].grad + 1.0), BAR, "dw accumulated onto ones " + tag)
    # ---- two identical calls: bit-identical (no atomics, fixed-order folds)
    f2 = c.kernel_forward(lib)
    for k in f:
        assert torch.equal(torch.nan_to_num(f[k]), torch.nan_to_num(f2[k])), k + " " + tag
    res2 = c.kernel_backward(lib, f)
    for k in res:
        assert torch.equal(torch.nan_to_num(res[k]), torch.nan_to_num(res2[k])), k + " " + tag


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_conv3x3_vs_f64(dev, case, norm):
    _check(dev, False, case, norm, 100 + sum(case) + int(norm))


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("case", DECONV_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_deconv_vs_f64(dev, case, norm):
    _check(dev, True, case, norm, 200 + sum(case) + int(norm))


def test_prep_orders(dev):
    """the two K-major orders of both families, element for element"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(4)
    w = torch.randn(64, 32, 3, 3, generator=g).to(dev)                                            # [co, ci, ty, tx]
    wd = torch.randn(32, 64, 2, 2, generator=g).to(dev)                                           # [ci, co, i, j]
    out = [_nan(w.numel(), dev=dev) for _ in range(2)] + [_nan(wd.numel(), dev=dev) for _ in range(2)]
    p2, i2 = ctypes.c_void_p * 2, ctypes.c_int * 2
    _lib.check(lib.papc_conv2d_prep_f32(p2(w.data_ptr(), wd.data_ptr()), p2(out[0].data_ptr(), out[2].data_ptr()), p2(out[1].data_ptr(), out[3].data_ptr()),
                                        i2(32, 32), i2(64, 64), i2(1, 2), i2(0, 1), 2, _lib.stream_ptr()), "prep")
    assert torch.equal(out[0].view(64, 9, 32), w.view(64, 32, 9).permute(0, 2, 1))               # wk [co][tap][ci]
    assert torch.equal(out[1].view(32, 9, 64), w.view(64, 32, 9).permute(1, 2, 0))               # wt [ci][tap][co]
    assert torch.equal(out[2].view(4, 64, 32), wd.view(32, 64, 4).permute(2, 1, 0))              # wk [ij][co][ci]
    assert torch.equal(out[3].view(32, 4, 64), wd.view(32, 64, 4).permute(0, 2, 1))              # wt [ci][ij][co]


def test_conv2d_ok_rejects_with_a_message(dev):
    lib = _lib.load()
    assert lib.papc_conv2d_ok(64, 64, 1, 1, 1) and lib.papc_conv2d_ok(256, 32, 2, 496, 432) and lib.papc_deconv2d_ok(256, 128, 4)
    for args, word in (((48, 64, 1, 8, 8), "Cin=48"), ((64, 64, 3, 8, 8), "stride 3"), ((64, 288, 1, 8, 8), "Cout=288")):
        assert lib.papc_conv2d_ok(*args) == 0, args
        assert word in lib.papc_last_error_string().decode(), (args, lib.papc_last_error_string())
    assert lib.papc_deconv2d_ok(64, 64, 3) == 0
    x, w, y, part = (torch.zeros(64 * 48, device=dev), torch.zeros(9 * 48 * 64, device=dev), _nan(64, 64, dev=dev), _nan(1, 2, 64, dev=dev))
    with pytest.raises(_lib.PapcError, match="Cin=48"):
        _lib.check(lib.papc_conv2d_fwd_f32(x.data_ptr(), 0, 0, w.data_ptr(), 1, 8, 8, 48, 64, 1, y.data_ptr(), part.data_ptr(), _lib.stream_ptr()), "conv fwd")
    assert bool(torch.isnan(y).all())                                                             # nothing was launched
