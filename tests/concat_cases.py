"""The concat-conv kernels against float64 on the materialised concat, written once for both kernel families: tests/test_gpu_pointnet_seg.py
runs it on papc_amd.segment.FAMILY (csrc/cloud_concat.hip), tests/test_gpu_vfe.py on papc_amd.vfe.FAMILY (csrc/cloud_concat_k.hip), each with
its own shapes and bar.  A family is a papc_amd.cloudconcat.Family: the names of its C entry points.  A plain helper module like
tests/detect_cases.py."""
import numpy as np
import torch

from papc_amd import _lib
from tests.util import assert_close


def _np(t):
    return t.detach().double().cpu().numpy()


def kernel_case(dev, B, N, cp, cg, cout, seed):
    """x, g, w, bias, dz, gamma, beta, (c1, c2): gamma negative on every fourth channel, random c1 / c2"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * N, cp, generator=g)
    gf = torch.relu(torch.randn(B, cg, generator=g))
    w = torch.randn(cout, cp + cg, generator=g) / np.sqrt(cp + cg)
    b = torch.randn(cout, generator=g) * 0.1
    dz = torch.randn(B * N, cout, generator=g)
    gamma = torch.rand(cout, generator=g) + 0.5
    gamma[::4] *= -1.0
    beta = torch.randn(cout, generator=g) * 0.2
    c12 = torch.randn(2, cout, generator=g) * 0.1
    return [t.to(dev) for t in (x, gf, w, b, dz, gamma, beta, c12)]


def fwd(fam, x, gf, w, b, B, N, stats=True):
    """-> y, the statistics partials (None without stats), cvec"""
    lib = _lib.load()
    dev = x.device
    cp, cg, cout = x.shape[1], gf.shape[1], w.shape[0]
    y = torch.empty(B * N, cout, device=dev)
    cvec = torch.empty(B, cout, device=dev)
    parts = getattr(lib, fam.parts)(B, N)
    st = torch.empty(parts, 2, cout, device=dev) if stats else None
    _lib.check(getattr(lib, fam.fwd)(x.data_ptr(), cp, gf.data_ptr(), w.data_ptr(), _lib.ptr(b), B, N, cp, cg, cout, y.data_ptr(), cvec.data_ptr(),
                                     _lib.ptr(st), _lib.stream_ptr()), fam.fwd)
    return y, st, cvec


def bwd(fam, consts, dz, y, x, gf, w, B, N, dx=None, accumulate=0):
    lib = _lib.load()
    dev = x.device
    cp, cg, cout = x.shape[1], gf.shape[1], w.shape[0]
    mean, invstd, scale, shift, c1, c2 = consts
    out = {"dx": dx if dx is not None else torch.empty(B * N, cp, device=dev), "dw": torch.empty(cout, cp + cg, device=dev),
           "db": torch.empty(cout, device=dev), "dg": torch.empty(B, cg, device=dev), "s": torch.empty(B, cout, device=dev)}
    nb = getattr(lib, fam.bwd_workspace)(B, N, cp, cg, cout)
    assert nb > 0
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    _lib.check(getattr(lib, fam.bwd)(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), c1.data_ptr(),
                                     c2.data_ptr(), x.data_ptr(), cp, gf.data_ptr(), w.data_ptr(), B, N, cp, cg, cout, out["dx"].data_ptr(), cp,
                                     accumulate, out["dw"].data_ptr(), out["db"].data_ptr(), out["dg"].data_ptr(), out["s"].data_ptr(), ws.data_ptr(),
                                     nb, _lib.stream_ptr()), fam.bwd)
    return out


def check_kernels_vs_f64(fam, dev, B, N, cp, cg, cout, seed, bar, tag, repeat_forward=False):
    """forward (y, the statistics partials) and backward (dX_p, dW_p, dW_g, d bias, s, dg) of one layer against float64; a second backward is
    bit-identical, `accumulate` adds dX_p to what the buffer holds, the forward without statistics gives the same y (repeat_forward: and so
    does a second forward with them, statistics included).  -> the forward's cvec"""
    x, gf, w, b, dz, gamma, beta, c12 = kernel_case(dev, B, N, cp, cg, cout, seed)
    y, stats, cvec = fwd(fam, x, gf, w, b, B, N)
    x64, g64, w64, b64 = (t.double() for t in (x, gf, w, b))           # (float64 on the device: the reference products)
    cat = torch.cat([x64, g64.repeat_interleave(N, 0)], 1)
    y_ref = cat @ w64.t() + b64
    assert_close(_np(y), _np(y_ref), bar, "concat conv y " + tag)
    s = stats.double().sum(0)
    assert_close(_np(s[0]), _np(y_ref.sum(0)), bar, "sum y " + tag)
    assert_close(_np(s[1]), _np((y_ref * y_ref).sum(0)), bar, "sum y^2 " + tag)
    # the backward, from this layer's BatchNorm constants (batch statistics of the kernel's own y) and the kernel's own y
    yk = y.double()
    mean = yk.mean(0)
    invstd = 1.0 / torch.sqrt(yk.var(0, unbiased=False) + 1e-5)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    consts = [t.float().contiguous() for t in (mean, invstd, scale, shift, c12[0].double(), c12[1].double())]
    m32, i32, sc32, sh32, k1, k2 = (t.double() for t in consts)
    p = torch.where(sc32 * yk + sh32 > 0, dz.double(), torch.zeros_like(yk))
    dY = sc32 * ((p - k1) - (yk - m32) * i32 * k2)
    out = bwd(fam, consts, dz, y, x, gf, w, B, N)
    s_ref = dY.view(B, N, cout).sum(1)
    assert_close(_np(out["dx"]), _np(dY @ w64[:, :cp]), bar, "dX_p " + tag)
    dw_ref = dY.t() @ cat
    assert_close(_np(out["dw"][:, :cp]), _np(dw_ref[:, :cp]), bar, "dW_p " + tag)
    assert_close(_np(out["dw"][:, cp:]), _np(dw_ref[:, cp:]), bar, "dW_g " + tag)
    assert_close(_np(out["db"]), _np(dY.sum(0)), bar, "d bias " + tag)
    assert_close(_np(out["s"]), _np(s_ref), bar, "s " + tag)
    assert_close(_np(out["dg"]), _np(s_ref @ w64[:, cp:]), bar, "dg " + tag)
    # two identical calls: bit-identical (no atomics, fixed-order folds); the accumulate flag adds dX to what the buffer holds
    again = bwd(fam, consts, dz, y, x, gf, w, B, N)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    if repeat_forward:
        y_again, stats_again, _ = fwd(fam, x, gf, w, b, B, N)
        assert torch.equal(y_again, y) and torch.equal(stats_again, stats)
    base = torch.randn(B * N, cp, generator=torch.Generator().manual_seed(5)).to(dev)
    acc = bwd(fam, consts, dz, y, x, gf, w, B, N, dx=base.clone(), accumulate=1)
    assert_close(_np(acc["dx"]), _np(base.double() + dY @ w64[:, :cp]), bar, "dX_p accumulated " + tag)
    # eval mode: no statistics, the same y
    y2, _, _ = fwd(fam, x, gf, w, b, B, N, stats=False)
    assert torch.equal(y2, y)
    return cvec
