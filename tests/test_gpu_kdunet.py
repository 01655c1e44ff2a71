"""GPU tests of the KDUNet part segmenter (papc_amd.models.KDUNet): the down-level kernels (csrc/kdbn.hip) against a float64 restatement of a
level (tests/kdunet_ref.py) over every path of the kernels and every way a tile can straddle the plane boundaries, the batch statistics at
the inputs the levels really see, the rejections, the whole model against float64 with the kernels' decisions pinned, bit-reproducible and
graph-replayable train steps, no library GEMM in a step, the error paths and a loader batch through to the loss."""
import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import head as H
from papc_amd import kdnet
from papc_amd.models import KDUNet
from tests import kdunet_ref
from tests.kd_cases import _np, _split_vectors
from tests.util import assert_close, copy_into_model, kernel_decisions, seeded_model_state

pytestmark = pytest.mark.gpu
BAR = 2e-4          # the project's model-level bar (as tests/test_gpu_kdnet.py)
NC = 50
EPS = kdunet_ref.EPS
MOM = kdunet_ref.MOMENTUM


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------

SHAPES = [(1024, 3, 32), (64, 32, 64), (16, 64, 256), (8, 256, 512), (4, 512, 1024)]
CASES = [(d, c, f, B) for (d, c, f) in SHAPES for B in (16, 19)] + [(2, 512, 1024, 33)]   # dim = 2, B = 33: a ragged last tile over many clouds


def _kernel_fwd(lib, x, sel, w, b, gamma, beta, rmean, rvar, B, dim, training=True):
    M, cin = x.shape
    f = w.shape[0] // 3
    dev = x.device
    res = {"out": torch.empty(M // 2, f, device=dev), "win": torch.empty(M // 2, f, device=dev, dtype=torch.uint8),
           "zhat": torch.empty(M // 2, f, device=dev), "mean": torch.empty(cin, device=dev), "tmat": torch.empty(3 * f, cin, device=dev),
           "stats": torch.empty(4, 3 * f, device=dev)}
    nb = lib.papc_kdbn_fwd_workspace(B, dim, cin, f)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    ss = 0 if sel.dim() == 1 else sel.stride(0)
    _lib.check(lib.papc_kdbn_fwd_f32(x.data_ptr(), x.stride(0), sel.data_ptr(), ss, w.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                     rmean.data_ptr(), rvar.data_ptr(), B, dim, cin, f, EPS, MOM, 1 if training else 0, res["out"].data_ptr(),
                                     res["win"].data_ptr(), res["zhat"].data_ptr(), res["mean"].data_ptr(), res["tmat"].data_ptr(),
                                     res["stats"].data_ptr(), ws.data_ptr(), nb, _lib.stream_ptr()), "papc_kdbn_fwd_f32")
    return res


def _kernel_bwd(lib, gout, fw, x, sel, w, gamma, B, dim):
    M, cin = x.shape
    f = w.shape[0] // 3
    dev = x.device
    nan = float("nan")
    res = {"dx": torch.full((M, cin), nan, device=dev), "dw": torch.full((3 * f, cin), nan, device=dev), "db": torch.full((3 * f,), nan, device=dev),
           "dgamma": torch.full((3 * f,), nan, device=dev), "dbeta": torch.full((3 * f,), nan, device=dev)}
    nb = lib.papc_kdbn_bwd_workspace(B, dim, cin, f)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    ss = 0 if sel.dim() == 1 else sel.stride(0)
    _lib.check(lib.papc_kdbn_bwd_f32(gout.data_ptr(), fw["out"].data_ptr(), fw["win"].data_ptr(), fw["zhat"].data_ptr(), x.data_ptr(), x.stride(0),
                                     sel.data_ptr(), ss, w.data_ptr(), gamma.data_ptr(), fw["mean"].data_ptr(), fw["tmat"].data_ptr(),
                                     fw["stats"].data_ptr(), B, dim, cin, f, 1, res["dx"].data_ptr(), cin, res["dw"].data_ptr(), res["db"].data_ptr(),
                                     res["dgamma"].data_ptr(), res["dbeta"].data_ptr(), 0, ws.data_ptr(), nb, _lib.stream_ptr()), "papc_kdbn_bwd_f32")
    return res


def _level_params(cin, f, g):
    w = torch.randn(3 * f, cin, generator=g) / np.sqrt(cin)
    b = torch.randn(3 * f, generator=g) * 0.1
    gamma = (torch.rand(3 * f, generator=g) + 0.5) * torch.where(torch.rand(3 * f, generator=g) < 0.25, -1.0, 1.0)
    beta = torch.randn(3 * f, generator=g) * 0.2
    rmean = torch.randn(3 * f, generator=g) * 0.3
    rvar = torch.rand(3 * f, generator=g) + 0.5
    return w, b, gamma, beta, rmean, rvar


def _modules(dev, cin, f, w, b, gamma, beta, rmean, rvar):
    conv, bn = torch.nn.Conv1d(cin, 3 * f, 1).to(dev), torch.nn.BatchNorm1d(3 * f, eps=EPS).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w.view(3 * f, cin, 1))
        conv.bias.copy_(b)
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rmean)
        bn.running_var.copy_(rvar)
    return conv, bn


@pytest.mark.parametrize("dim,cin,f,B", CASES)
def test_kdbn_kernels_vs_f64(dev, dim, cin, f, B):
    lib = _lib.load()
    assert kdnet.bn_kernel_ok(dim, cin, f) and B * dim >= 64
    g = torch.Generator().manual_seed(dim * 7 + cin + f + B)
    x = torch.randn(B * dim, cin, generator=g)
    w, b, gamma, beta, rmean, rvar = _level_params(cin, f, g)
    gout = torch.randn(B * dim // 2, f, generator=g)
    xd, wd, bd, gad, bed, gd = (t.to(dev) for t in (x, w, b, gamma, beta, gout))
    for name, sel in _split_vectors(B, dim, dim + B):
        tag = "%s dim=%d Cin=%d F=%d B=%d" % (name, dim, cin, f, B)
        seld = torch.from_numpy(sel.astype(np.int32)).to(dev)
        rm, rv = rmean.to(dev), rvar.to(dev)
        fw = _kernel_fwd(lib, xd, seld, wd, bd, gad, bed, rm, rv, B, dim)
        out, win = fw["out"], fw["win"]
        leaf = lambda t: t.double().requires_grad_(True)      # noqa: E731
        x64, w64, b64, ga64, be64 = leaf(x), leaf(w), leaf(b), leaf(gamma), leaf(beta)
        ref, _, _, mean64, var64, _ = kdunet_ref.level(x64, sel, w64, b64, ga64, be64, B, dim)
        assert_close(_np(out), _np(ref), BAR, "out " + tag)
        assert set(np.unique(win.cpu().numpy())) <= {0, 1}
        assert_close(_np(fw["stats"][2]), _np(mean64), BAR, "mu " + tag)
        assert_close(_np(fw["stats"][1]), _np(1.0 / torch.sqrt(var64 + EPS)), BAR, "1/sigma " + tag)
        assert_close(_np(rm), _np(MOM * rmean.double() + (1 - MOM) * mean64), BAR, "running mean " + tag)
        assert_close(_np(rv), _np(MOM * rvar.double() + (1 - MOM) * var64), BAR, "running var " + tag)
        # the backward against float64 routed by the kernel's own decisions (winner bytes, out > 0)
        pinned = kdunet_ref.level(x64, sel, w64, b64, ga64, be64, B, dim, dec=(win.cpu(), (out > 0).cpu()))
        assert_close(_np(fw["zhat"])[_np(out) > 0], _np(pinned[5])[_np(out) > 0], BAR, "zhat " + tag)
        pinned[0].backward(gout.double())
        res = _kernel_bwd(lib, gd, fw, xd, seld, wd, gad, B, dim)
        assert_close(_np(res["dx"]), _np(x64.grad), BAR, "dX " + tag)
        assert_close(_np(res["dw"]), _np(w64.grad), BAR, "dW " + tag)
        assert_close(_np(res["dgamma"]), _np(ga64.grad), BAR, "dgamma " + tag)
        assert_close(_np(res["dbeta"]), _np(be64.grad), BAR, "dbeta " + tag)
        # the conv bias cancels in the norm: zero, on the scale of dbeta
        assert float(res["db"].abs().max()) <= BAR * float(be64.grad.abs().max()), "d bias " + tag
        # two identical calls: bit-identical (no atomics, fixed-order folds)
        again = _kernel_bwd(lib, gd, fw, xd, seld, wd, gad, B, dim)
        for k in res:
            assert torch.equal(res[k], again[k]), k + " " + tag
        # the torch-op path (PAPC_KDCONV=0): the same out
        conv, bn = _modules(dev, cin, f, w, b, gamma, beta, rmean, rvar)
        assert_close(_np(kdnet._kdconv_bn_torch(xd, seld, conv, bn, B, dim, True)), _np(ref), BAR, "torch-op out " + tag)


def _post_relu_rows(M, cin, seed):
    """what a level really sees: |N(0, 1)| plus a per-channel offset from [0, 2] -- post-ReLU, all positive, the mean up to about 3 sigma"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, cin, generator=g).abs() + 2.0 * torch.rand(cin, generator=g)


def test_statistics_at_post_relu_inputs(dev):
    """mu and var per channel from the rows' moments (w . xm + b, w^T C w / M) at offset, all-positive rows: this decides between the moments
    route and a no-store pass over the full conv"""
    lib = _lib.load()
    dim, cin, f, B = 64, 512, 1024, 2
    g = torch.Generator().manual_seed(77)
    x = _post_relu_rows(B * dim, cin, 78)
    w, b, gamma, beta, rmean, rvar = _level_params(cin, f, g)
    y = x.double() @ w.double().t() + b.double()
    mean64, var64 = y.mean(0), y.var(0, unbiased=False)
    assert float(var64.min()) > 100 * EPS, float(var64.min())        # the bar measures the kernel, not the conditioning
    sel = torch.randint(0, 3, (B, dim), generator=g).int().to(dev)
    fw = _kernel_fwd(lib, x.to(dev), sel, *(t.to(dev) for t in (w, b, gamma, beta, rmean, rvar)), B, dim)
    assert_close(_np(fw["stats"][2]), _np(mean64), BAR, "mu at post-ReLU rows")
    assert_close(_np(fw["stats"][3]), _np(var64), BAR, "var at post-ReLU rows")


def test_eval_mode_node_vs_f64(dev, monkeypatch):
    """eval mode: the norm is a fixed affine map of the running statistics -- the node's forward and every gradient (the conv bias now has one)"""
    monkeypatch.setattr(kdnet, "_KDCONV", True)
    B, dim, cin, f = 5, 16, 64, 96
    g = torch.Generator().manual_seed(13)
    x = torch.randn(B * dim, cin, generator=g)
    w, b, gamma, beta, rmean, rvar = _level_params(cin, f, g)
    sel = torch.randint(0, 3, (B, dim), generator=g)
    gout = torch.randn(B * dim // 2, f, generator=g)
    conv, bn = _modules(dev, cin, f, w, b, gamma, beta, rmean, rvar)
    xd = x.to(dev).requires_grad_(True)
    out = kdnet.kdconv_bn(xd, sel.int().to(dev), conv, bn, B, dim, False)
    assert type(out.grad_fn).__name__ == "_KDConvBNBackward"
    assert torch.equal(bn.running_mean.cpu(), rmean) and torch.equal(bn.running_var.cpu(), rvar)          # untouched
    leaf = lambda t: t.double().requires_grad_(True)      # noqa: E731
    x64, w64, b64, ga64, be64 = leaf(x), leaf(w), leaf(b), leaf(gamma), leaf(beta)
    dec = (out.grad_fn.saved_tensors[5].cpu(), (out.detach() > 0).cpu())
    ref = kdunet_ref.level(x64, sel.numpy(), w64, b64, ga64, be64, B, dim, dec=dec, running=(rmean.double(), rvar.double()))[0]
    assert_close(_np(out), _np(ref), BAR, "eval out")
    out.backward(gout.to(dev))
    ref.backward(gout.double())
    for name, got, want in (("dX", xd.grad, x64.grad), ("dW", conv.weight.grad.view(3 * f, cin), w64.grad), ("d bias", conv.bias.grad, b64.grad),
                            ("dgamma", bn.weight.grad, ga64.grad), ("dbeta", bn.bias.grad, be64.grad)):
        assert_close(_np(got), _np(want), BAR, "eval " + name)


def test_kdbn_clamps_bad_split_values(dev):
    """a split value outside 0..2 on the device is clamped: it cannot address outside the buffers"""
    lib = _lib.load()
    B, dim, cin, f = 2, 32, 32, 32
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B * dim, cin, generator=g).to(dev)
    ps = [t.to(dev) for t in _level_params(cin, f, g)]
    sel = torch.randint(0, 3, (B, dim), generator=g).int()
    bad = sel.clone()
    bad[sel == 0] = -7
    bad[sel == 2] = 1 << 20
    gout = torch.randn(B * dim // 2, f, generator=g).to(dev)
    a = _kernel_fwd(lib, x, sel.to(dev), *[p.clone() for p in ps], B, dim)
    c = _kernel_fwd(lib, x, bad.to(dev), *[p.clone() for p in ps], B, dim)
    assert torch.equal(a["out"], c["out"]) and torch.equal(a["win"], c["win"])
    ra, rc = _kernel_bwd(lib, gout, a, x, sel.to(dev), ps[0], ps[2], B, dim), _kernel_bwd(lib, gout, c, x, bad.to(dev), ps[0], ps[2], B, dim)
    for k in ra:
        assert torch.equal(ra[k], rc[k]), k


@pytest.mark.parametrize("dim,cin,f,B", [(32, 32, 32, 3),       # M = 96: ragged against the 128-row dW chunk
                                          (2, 64, 64, 33)])      # M = 66: a ragged last 32-row tile over many clouds; Cin != F
def test_identity_norm_level_is_kdconv_bit_for_bit(dev, dim, cin, f, B):
    """With the norm set to the identity a kdbn level is a kdconv level, and the two families run the same bodies (csrc/kdlevel.h): eval mode
    with eps = 0, running_var = 1, running_mean = bias (zoff = +0 and 1/sigma = 1 exactly), gamma = 1, beta = bias.  (acc - 0) * 1,
    1 * z + beta and g * 1 are exact, and both dW paths fold the same chunk partials in the same order, so out, win, dX, dW and the bias
    gradient (kdbn's d bias and its dbeta) equal kdconv's bit for bit.  Cin = 3 is left out on purpose: kdconv starts its fmaf chain from the
    bias, kdbn from w0 x0 without one, and the two round differently."""
    lib = _lib.load()
    assert kdnet.bn_kernel_ok(dim, cin, f) and kdnet.kernel_ok(dim, cin, f)
    g = torch.Generator().manual_seed(dim * 7 + cin + f + B)
    M = B * dim
    x = torch.randn(M, cin, generator=g).to(dev)
    w = (torch.randn(3 * f, cin, generator=g) / np.sqrt(cin)).to(dev)
    b = (torch.randn(3 * f, generator=g) * 0.1).to(dev)
    gout = torch.randn(M // 2, f, generator=g).to(dev)
    one = torch.ones(3 * f, device=dev)
    st = _lib.stream_ptr()
    nan = float("nan")
    for name, sel in _split_vectors(B, dim, dim + B)[:2]:          # a shared sel [dim] and a per-cloud sel [B, dim]
        tag = "%s dim=%d Cin=%d F=%d B=%d" % (name, dim, cin, f, B)
        seld = torch.from_numpy(sel.astype(np.int32)).to(dev)
        ss = 0 if seld.dim() == 1 else seld.stride(0)
        # kdconv
        out_c, win_c = torch.empty(M // 2, f, device=dev), torch.empty(M // 2, f, device=dev, dtype=torch.uint8)
        _lib.check(lib.papc_kdconv_fwd_f32(x.data_ptr(), cin, seld.data_ptr(), ss, w.data_ptr(), b.data_ptr(), B, dim, cin, f, out_c.data_ptr(),
                                           win_c.data_ptr(), st), "papc_kdconv_fwd_f32")
        dx_c, dw_c, db_c = torch.full((M, cin), nan, device=dev), torch.full((3 * f, cin), nan, device=dev), torch.full((3 * f,), nan, device=dev)
        nb = lib.papc_kdconv_bwd_workspace(B, dim, cin, f)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        _lib.check(lib.papc_kdconv_bwd_f32(gout.data_ptr(), out_c.data_ptr(), win_c.data_ptr(), x.data_ptr(), cin, seld.data_ptr(), ss, w.data_ptr(), B,
                                           dim, cin, f, dx_c.data_ptr(), cin, dw_c.data_ptr(), db_c.data_ptr(), 0, ws.data_ptr(), nb, st),
                   "papc_kdconv_bwd_f32")
        # kdbn in eval mode, the norm the identity
        rmean, rvar = b.clone(), one.clone()
        out_b, win_b = torch.empty(M // 2, f, device=dev), torch.empty(M // 2, f, device=dev, dtype=torch.uint8)
        zhat, mean, tmat, stats = (torch.empty(M // 2, f, device=dev), torch.zeros(cin, device=dev), torch.zeros(3 * f, cin, device=dev),
                                   torch.empty(4, 3 * f, device=dev))
        nb = lib.papc_kdbn_fwd_workspace(B, dim, cin, f)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        _lib.check(lib.papc_kdbn_fwd_f32(x.data_ptr(), cin, seld.data_ptr(), ss, w.data_ptr(), b.data_ptr(), one.data_ptr(), b.data_ptr(),
                                         rmean.data_ptr(), rvar.data_ptr(), B, dim, cin, f, 0.0, MOM, 0, out_b.data_ptr(), win_b.data_ptr(),
                                         zhat.data_ptr(), mean.data_ptr(), tmat.data_ptr(), stats.data_ptr(), ws.data_ptr(), nb, st), "papc_kdbn_fwd_f32")
        assert torch.equal(stats[0], torch.zeros_like(stats[0])) and torch.equal(stats[1], one), "the norm is not the identity " + tag
        dx_b, dw_b = torch.full((M, cin), nan, device=dev), torch.full((3 * f, cin), nan, device=dev)
        db_b, dgamma, dbeta = (torch.full((3 * f,), nan, device=dev) for _ in range(3))
        nb = lib.papc_kdbn_bwd_workspace(B, dim, cin, f)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        _lib.check(lib.papc_kdbn_bwd_f32(gout.data_ptr(), out_b.data_ptr(), win_b.data_ptr(), zhat.data_ptr(), x.data_ptr(), cin, seld.data_ptr(), ss,
                                         w.data_ptr(), one.data_ptr(), mean.data_ptr(), tmat.data_ptr(), stats.data_ptr(), B, dim, cin, f, 0,
                                         dx_b.data_ptr(), cin, dw_b.data_ptr(), db_b.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), 0, ws.data_ptr(), nb,
                                         st), "papc_kdbn_bwd_f32")
        assert float(out_c.abs().max()) > 0 and float(dw_c.abs().max()) > 0 and float(dx_c.abs().max()) > 0, tag
        for what, got, want in (("out", out_b, out_c), ("win", win_b, win_c), ("dX", dx_b, dx_c), ("dW", dw_b, dw_c), ("d bias", db_b, db_c),
                                ("dbeta", dbeta, db_c)):
            assert torch.equal(got, want), "%s of the identity-norm kdbn level differs from kdconv's, %s" % (what, tag)


def test_shapes_outside_kdbn_ok(dev):
    lib = _lib.load()
    t = torch.zeros(1 << 16, device=dev)
    p = t.data_ptr()
    st = _lib.stream_ptr()
    for dim, cin, f, what in ((33, 32, 32, "dim=33"), (32, 48, 32, "Cin=48"), (32, 32, 40, "F=40"), (32, 32, 1056, "F=1056")):
        assert not kdnet.bn_kernel_ok(dim, cin, f)
        fwd = lambda: lib.papc_kdbn_fwd_f32(p, cin, p, 0, p, p, p, p, p, p, 1, dim, cin, f, EPS, MOM, 1, p, p, p, p, p, p, p, 1 << 18, st)   # noqa: E731
        bwd = lambda: lib.papc_kdbn_bwd_f32(p, p, p, p, p, cin, p, 0, p, p, p, p, p, 1, dim, cin, f, 1, p, cin, p, p, p, p, 0, p, 1 << 18, st)   # noqa: E731
        for call in (fwd, bwd):
            assert call() == -2                                                                   # PAPC_E_UNSUPPORTED
            with pytest.raises(_lib.PapcError, match=what):
                _lib.check(call(), "kdbn")
    assert kdnet.bn_kernel_ok(64, 512, 1024) and not kdnet.kernel_ok(64, 512, 1024)              # F = 1024: beyond kdconv's 512
    # kdconv_bn takes the torch-op path there and agrees with float64
    B, dim, cin, f = 4, 32, 48, 32
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B * dim, cin, generator=g)
    w, b, gamma, beta, rmean, rvar = _level_params(cin, f, g)
    sel = torch.randint(0, 3, (B, dim), generator=g)
    conv, bn = _modules(dev, cin, f, w, b, gamma, beta, rmean, rvar)
    out = kdnet.kdconv_bn(x.to(dev), sel.int().to(dev), conv, bn, B, dim, True)
    ref = kdunet_ref.level(x.double(), sel.numpy(), w.double(), b.double(), gamma.double(), beta.double(), B, dim)
    assert type(out.grad_fn).__name__ != "_KDConvBNBackward"
    assert_close(_np(out), _np(ref[0]), BAR, "torch-op path at Cin=48")
    assert_close(_np(bn.running_var), _np(MOM * rvar.double() + (1 - MOM) * ref[4]), BAR, "torch-op running var")


# ---- the model --------------------------------------------------------------------------------------------------------------------------

def _seeded_model(dev, seed):
    m = KDUNet(num_classes=NC).to(dev)
    copy_into_model(m, seeded_model_state(m, seed))
    return m.train()


def _inputs(B, seed, per_cloud=True):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, 3, 1024)).astype(np.float32)
    sels = [rng.integers(0, 3, size=(B, d) if per_cloud else (d,)) for d in kdnet.DIMS]
    y = rng.integers(0, NC, size=(B, 1024, 1))
    return x, sels, y


def _recording(monkeypatch):
    """record every down level's output and every up stack's output of a forward (their autograd nodes hold the kernels' decisions)"""
    down, up = [], []
    inner_level, inner_cbr = kdnet.kdconv_bn, KDUNet._cbr

    def level(*a, **k):
        out = inner_level(*a, **k)
        down.append(out)
        return out

    def cbr(self, blocks, *a, **k):
        out = inner_cbr(self, blocks, *a, **k)
        up.append((len(blocks), out))
        return out
    monkeypatch.setattr(kdnet, "kdconv_bn", level)
    monkeypatch.setattr(KDUNet, "_cbr", cbr)
    return down, up


@pytest.mark.parametrize("form", ["per-cloud packed", "five shared arrays"])
def test_model_vs_f64(dev, monkeypatch, form):
    monkeypatch.setattr(kdnet, "_KDCONV", True)
    B = 2
    m = _seeded_model(dev, 31)
    per_cloud = form == "per-cloud packed"
    x, sels, y = _inputs(B, 3, per_cloud=per_cloud)
    down, up = _recording(monkeypatch)
    if per_cloud:
        split = torch.from_numpy(np.concatenate(sels, axis=1).astype(np.int32)).to(dev)          # the packed form [B, 2046]
        logits = m([torch.from_numpy(x).to(dev), split])
    else:
        logits = m([x, [s.astype(np.int64) for s in sels[:5]]])                                  # numpy points, just the five levels read
    assert logits.shape == (B, 1024, NC) and len(down) == 5 and len(up) == 5
    dec, up_dec = [], {}
    for out in down:
        assert type(out.grad_fn).__name__ == "_KDConvBNBackward"
        dec.append((out.grad_fn.saved_tensors[5].cpu(), (out.detach() > 0).cpu()))
    for i, (L, out) in enumerate(up):
        _, alive, masks = kernel_decisions(out)
        up_dec[(i + 1, L - 1)] = alive.cpu()
        if L == 2 and masks[0] is not None:
            up_dec[(i + 1, 0)] = masks[0].cpu()
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.named_parameters()}
    ref, stats = kdunet_ref.kdunet(P, torch.from_numpy(x).double(), sels[:5], dec=dec, up_dec=up_dec)
    assert_close(_np(logits), _np(ref), BAR, "logits " + form)
    yd = torch.from_numpy(y.reshape(-1)).to(dev)
    loss = H.softmax_cross_entropy(logits.view(-1, NC), yd)
    ref_loss = torch.nn.functional.cross_entropy(ref.view(-1, NC), torch.from_numpy(y.reshape(-1)))
    assert_close(_np(loss), _np(ref_loss), BAR, "loss " + form)
    loss.backward(H.unit_gradient(dev))
    ref_loss.backward()
    bad = []
    named = dict(m.named_parameters())
    for k, p in named.items():
        assert p.grad is not None, k
        try:
            # A per-channel constant ahead of a train-mode norm cancels in it: its gradient is zero in exact arithmetic (float64 leaves 1e-18)
            # and a relative bar has no scale to read.  A conv bias is held to zero on the scale of its norm's dbeta; a deconv bias (the
            # deconv output goes through the concat into ConvBNReLU) on the scale of the deconv's weight gradient, a sum of the same
            # per-row terms times O(1) activations.
            if k.endswith("_conv.bias") or (".deconv" in k and k.endswith(".bias")):
                other = k.replace("_conv.bias", "_batch_norm.bias") if k.endswith("_conv.bias") else k.replace(".bias", ".weight")
                scale = float(P[other].grad.abs().max())
                assert float(p.grad.abs().max()) <= BAR * scale, "d %s: %.3e on the scale %.3e" % (k, float(p.grad.abs().max()), scale)
            else:
                assert_close(_np(p.grad), _np(P[k].grad), BAR, "d %s %s" % (k, form))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad
    # the running statistics: started from (0, 1), one train-mode forward
    for n, (mean, var) in stats.items():
        bn = m.get_submodule(n)
        assert_close(_np(bn.running_mean), _np((1 - MOM) * mean), BAR, "running mean " + n)
        assert_close(_np(bn.running_var), _np(MOM + (1 - MOM) * var), BAR, "running var " + n)
    # eval mode: the logits through the running statistics
    m.eval()
    running = {k: v.detach().double().cpu() for k, v in m.named_buffers() if "running" in k}
    with torch.no_grad():
        ev = m([torch.from_numpy(x).to(dev), [torch.from_numpy(s.astype(np.int32)).to(dev) for s in sels]])
        ref_ev, _ = kdunet_ref.kdunet({k: v.detach() for k, v in P.items()}, torch.from_numpy(x).double(), sels[:5], running=running)
    assert_close(_np(ev), _np(ref_ev), BAR, "eval logits " + form)


def _train_setup(dev, B=4, seed=5):
    from papc_amd.distributed import FlatAdam, FlatParams
    torch.manual_seed(seed)
    m = KDUNet(num_classes=NC).to(dev).train()
    flat = FlatParams(m)
    opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)
    x, sels, y = _inputs(B, seed)
    xd = torch.from_numpy(x).to(dev)
    split = kdnet.pack_split_dims(sels, B, dev)
    return m, flat, opt, xd, split, torch.from_numpy(y.reshape(-1)).to(dev)


def _step(m, opt, x, split, y):
    logits = m([x, split])
    loss = H.softmax_cross_entropy(logits.view(-1, NC), y)
    loss.backward(H.unit_gradient(x.device))
    opt.step_dev(1.0, zero_grad=True, self_tick=True)


def _state(m, flat, opt):
    return [flat.data, flat.grad, opt.m, opt.v, opt.t_dev] + [b for _, b in m.named_buffers() if b.dtype == torch.float32]


def test_train_step_bit_reproducible_and_graph_replay_equal(dev, monkeypatch):
    monkeypatch.setattr(kdnet, "_KDCONV", True)
    m, flat, opt, x, split, y = _train_setup(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                     # warm-up (eager, side stream) before the capture
            _step(m, opt, x, split, y)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    snap = [t.clone() for t in _state(m, flat, opt)]

    def restore():
        with torch.no_grad():
            for t, v in zip(_state(m, flat, opt), snap):
                t.copy_(v)
        torch.cuda.synchronize()

    _step(m, opt, x, split, y)
    torch.cuda.synchronize()
    eager1 = [t.clone() for t in _state(m, flat, opt)]
    restore()
    _step(m, opt, x, split, y)
    torch.cuda.synchronize()
    eager2 = [t.clone() for t in _state(m, flat, opt)]
    for a, b in zip(eager1, eager2):
        assert torch.equal(a, b), "two identical train steps differ"
    assert not torch.equal(eager1[0], snap[0])          # the step did move the parameters
    restore()
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _step(m, opt, x, split, y)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    restore()
    g.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(eager1, _state(m, flat, opt))):
        assert torch.equal(a, b), "graph replay differs from the eager step (state tensor %d)" % i


def test_train_step_runs_no_library_gemm(dev, monkeypatch):
    from torch.profiler import ProfilerActivity, profile
    monkeypatch.setattr(kdnet, "_KDCONV", True)
    m, flat, opt, x, split, y = _train_setup(dev)
    _step(m, opt, x, split, y)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        _step(m, opt, x, split, y)
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    gemmish = ("cijk", "gemm", "gemv", "bmm", "matmul", "rocblas", "hipblas", "tensile", "mfma")
    mine = lambda n: "papc::" in n.split("(")[0] or n.startswith("_ZN4papc")      # (demangled or not)
    ours = [n for n in names if mine(n)]
    for k in ("kb_gram_kernel", "kb_gram3_kernel", "kb_t_kernel", "kb_finalize_kernel", "kb_fwd_kernel", "kb_fwd3_kernel", "kb_dw_kernel",
              "kb_dw3_kernel", "kb_a_kernel", "kb_dx_kernel"):
        assert any(k in n for n in ours), (k, sorted(names))
    foreign = [n for n in names if not mine(n) and any(s in n.lower() for s in gemmish)]
    assert not foreign, foreign


def test_errors(dev):
    m = KDUNet(num_classes=NC).to(dev)
    x, sels, _ = _inputs(2, 1)
    with pytest.raises(_lib.PapcError, match="1000.*1024|1024.*1000"):
        m([torch.zeros(2, 3, 1000, device=dev), sels])
    with pytest.raises(_lib.PapcError):
        m([torch.from_numpy(x), sels])                      # a CPU tensor
    with pytest.raises(_lib.PapcError, match="7 levels"):
        m([x, sels[:7]])                                    # neither the ten levels nor the first five
    with pytest.raises(_lib.PapcError, match="shape"):
        m([x, [s[:, :-1] for s in sels[:5]]])               # levels of the wrong length
    with pytest.raises(_lib.PapcError, match="integer"):
        m([x, [s.astype(np.float32) for s in sels]])        # the wrong dtype
    with pytest.raises(_lib.PapcError, match="integer"):
        m([x, torch.zeros(2, kdnet.PACKED, device=dev)])
    bad = [s.copy() for s in sels]
    bad[4][1, 7] = 3
    with pytest.raises(_lib.PapcError, match="0, 1 or 2"):
        m([x, bad])                                         # a split value of 3 in a numpy list
    conv, bn = torch.nn.Conv1d(32, 96, 1).to(dev), torch.nn.BatchNorm1d(96).to(dev)
    with pytest.raises(_lib.PapcError):
        kdnet.kdconv_bn(torch.zeros(64, 32, device=dev, dtype=torch.float64), torch.zeros(32, device=dev, dtype=torch.int32), conv, bn, 2, 32, True)
    with pytest.raises(_lib.PapcError):
        kdnet.kdconv_bn(torch.zeros(64, 32, device=dev), torch.zeros(32, device=dev, dtype=torch.int64), conv, bn, 2, 32, True)
    with pytest.raises(_lib.PapcError):
        kdnet.kdconv_bn(torch.zeros(64, 32), torch.zeros(32, dtype=torch.int32), conv, bn, 2, 32, True)


def test_loader_batch_to_loss(dev):
    from papc_amd.datasets import KDSegDataLoader
    rng = np.random.default_rng(21)

    def opener(path):           # a small synthetic ShapeNet-part file (the loader's h5 keys)
        return {"data": rng.normal(size=(1, 1024, 3)).astype(np.float32), "pid": rng.integers(0, NC, size=(1, 1024))}
    gen = KDSegDataLoader(max_point=1024, batchsize=2, path="shapenet", mode="test", opener=opener)
    batch, label = next(iter(gen()))
    assert label.shape == (2, 1024, 1)
    m = _seeded_model(dev, 55)
    logits = m(batch)                                       # the loader's [points, packed split dims] batch, as it comes
    assert logits.shape == (2, 1024, NC)
    loss = H.softmax_cross_entropy(logits.view(-1, NC), torch.from_numpy(label.reshape(-1)).to(dev))
    loss.backward(H.unit_gradient(dev))
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
