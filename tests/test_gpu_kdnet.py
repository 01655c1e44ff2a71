"""GPU tests of the KD-Net classifier (papc_amd.models.KDNet): the kdconv kernels (csrc/kdconv.hip) against a float64 restatement of a level
(tests/kdnet_ref.py) over every path of the kernels and every way a tile can straddle the plane boundaries, the rejections, the whole model
against float64 with the kernels' decisions pinned, agreement with the torch-op path (PAPC_KDCONV=0), bit-reproducible and graph-replayable
train steps, no library GEMM in a step, the error paths and a loader batch through to the loss."""
import copy

import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import head as H
from papc_amd import kdnet
from papc_amd.models import KDNet
from tests import kdnet_ref
from tests.kd_cases import _np, _split_vectors
from tests.util import assert_close, copy_into_model, seeded_model_state

pytestmark = pytest.mark.gpu
BAR = 2e-4          # the project's model-level bar (as tests/test_gpu_pointnet.py)
NC = 10


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------

SHAPES = [(1024, 3, 32), (512, 32, 64), (64, 128, 128), (32, 128, 256), (8, 256, 512), (4, 512, 512), (2, 512, 128)]
CASES = [(d, c, f, B) for (d, c, f) in SHAPES for B in (1, 3)] + [(2, 512, 128, 33)]      # dim = 2, B = 33: a ragged last tile over many clouds


def _kernel_fwd(lib, x, sel, w, b, B, dim):
    M, cin = x.shape
    f = w.shape[0] // 3
    out = torch.empty(M // 2, f, device=x.device)
    win = torch.empty(M // 2, f, device=x.device, dtype=torch.uint8)
    ss = 0 if sel.dim() == 1 else sel.stride(0)
    _lib.check(lib.papc_kdconv_fwd_f32(x.data_ptr(), x.stride(0), sel.data_ptr(), ss, w.data_ptr(), b.data_ptr(), B, dim, cin, f, out.data_ptr(),
                                       win.data_ptr(), _lib.stream_ptr()), "papc_kdconv_fwd_f32")
    return out, win


def _kernel_bwd(lib, gout, out, win, x, sel, w, B, dim):
    M, cin = x.shape
    f = w.shape[0] // 3
    dev = x.device
    res = {"dx": torch.full((M, cin), float("nan"), device=dev), "dw": torch.empty(3 * f, cin, device=dev), "db": torch.empty(3 * f, device=dev)}
    nb = lib.papc_kdconv_bwd_workspace(B, dim, cin, f)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    ss = 0 if sel.dim() == 1 else sel.stride(0)
    _lib.check(lib.papc_kdconv_bwd_f32(gout.data_ptr(), out.data_ptr(), win.data_ptr(), x.data_ptr(), x.stride(0), sel.data_ptr(), ss, w.data_ptr(), B, dim,
                                       cin, f, res["dx"].data_ptr(), cin, res["dw"].data_ptr(), res["db"].data_ptr(), 0, ws.data_ptr(), nb,
                                       _lib.stream_ptr()), "papc_kdconv_bwd_f32")
    return res


@pytest.mark.parametrize("dim,cin,f,B", CASES)
def test_kdconv_kernels_vs_f64(dev, dim, cin, f, B):
    lib = _lib.load()
    assert kdnet.kernel_ok(dim, cin, f)
    g = torch.Generator().manual_seed(dim * 7 + cin + f + B)
    x = torch.randn(B * dim, cin, generator=g)
    w = torch.randn(3 * f, cin, generator=g) / np.sqrt(cin)
    b = torch.randn(3 * f, generator=g) * 0.1
    gout = torch.randn(B * dim // 2, f, generator=g)
    xd, wd, bd, gd = (t.to(dev) for t in (x, w, b, gout))
    conv = torch.nn.Conv1d(cin, 3 * f, 1).to(dev)
    with torch.no_grad():
        conv.weight.copy_(wd.view(3 * f, cin, 1))
        conv.bias.copy_(bd)
    for name, sel in _split_vectors(B, dim, dim + B):
        tag = "%s dim=%d Cin=%d F=%d B=%d" % (name, dim, cin, f, B)
        seld = torch.from_numpy(sel.astype(np.int32)).to(dev)
        out, win = _kernel_fwd(lib, xd, seld, wd, bd, B, dim)
        x64, w64, b64 = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
        ref, _, _ = kdnet_ref.level(x64, sel, w64, b64, B, dim)
        assert_close(_np(out), _np(ref), BAR, "out " + tag)
        assert set(np.unique(win.cpu().numpy())) <= {0, 1}
        # the backward against float64 routed by the kernel's own decisions (winner bytes, out > 0)
        pinned, _, _ = kdnet_ref.level(x64, sel, w64, b64, B, dim, dec=(win.cpu(), (out > 0).cpu()))
        pinned.backward(gout.double())
        res = _kernel_bwd(lib, gd, out, win, xd, seld, wd, B, dim)
        assert_close(_np(res["dx"]), _np(x64.grad), BAR, "dX " + tag)
        assert_close(_np(res["dw"]), _np(w64.grad), BAR, "dW " + tag)
        assert_close(_np(res["db"]), _np(b64.grad), BAR, "db " + tag)
        # source points that feed no row: exact zeros
        fed = kdnet_ref.fed_points(sel, B, dim).reshape(-1)
        assert bool((res["dx"].cpu()[torch.from_numpy(~fed)] == 0).all()), "dX of unfed points " + tag
        # two identical calls: bit-identical (no atomics, fixed-order folds)
        again = _kernel_bwd(lib, gd, out, win, xd, seld, wd, B, dim)
        for k in res:
            assert torch.equal(res[k], again[k]), k + " " + tag
        # the torch-op path (PAPC_KDCONV=0): the same out
        assert_close(_np(kdnet._kdconv_torch(xd, seld, conv, B, dim)), _np(ref), BAR, "torch-op out " + tag)
    # about 28 % of the source points feed no row under random split dims (the share the issue states), at sizes where that is a statistic
    if dim >= 512:
        share = 1.0 - kdnet_ref.fed_points(_split_vectors(B, dim, 1)[1][1], B, dim).mean()
        assert 0.2 < share < 0.36, share


def test_kdconv_clamps_bad_split_values(dev):
    """a split value outside 0..2 on the device is clamped: it cannot address outside the buffers"""
    lib = _lib.load()
    B, dim, cin, f = 2, 32, 32, 32
    g = torch.Generator().manual_seed(4)
    x, w, b = torch.randn(B * dim, cin, generator=g).to(dev), torch.randn(3 * f, cin, generator=g).to(dev), torch.randn(3 * f, generator=g).to(dev)
    sel = torch.randint(0, 3, (B, dim), generator=g).int()
    bad = sel.clone()
    bad[sel == 0] = -7
    bad[sel == 2] = 1 << 20
    out_a, win_a = _kernel_fwd(lib, x, sel.to(dev), w, b, B, dim)
    out_b, win_b = _kernel_fwd(lib, x, bad.to(dev), w, b, B, dim)
    assert torch.equal(out_a, out_b) and torch.equal(win_a, win_b)


def test_kdconv_rejects_other_shapes(dev):
    lib = _lib.load()
    t = torch.zeros(1 << 16, device=dev)
    p = t.data_ptr()
    for dim, cin, f, what in ((33, 32, 32, "dim=33"), (32, 48, 32, "Cin=48"), (32, 32, 40, "F=40")):
        assert not kdnet.kernel_ok(dim, cin, f)
        assert lib.papc_kdconv_fwd_f32(p, cin, p, 0, p, p, 1, dim, cin, f, p, p, _lib.stream_ptr()) == -2          # PAPC_E_UNSUPPORTED
        with pytest.raises(_lib.PapcError, match=what):
            _lib.check(lib.papc_kdconv_fwd_f32(p, cin, p, 0, p, p, 1, dim, cin, f, p, p, _lib.stream_ptr()), "fwd")
        assert lib.papc_kdconv_bwd_f32(p, p, p, p, cin, p, 0, p, 1, dim, cin, f, p, cin, p, p, 0, p, 1 << 18, _lib.stream_ptr()) == -2
        with pytest.raises(_lib.PapcError, match=what):
            _lib.check(lib.papc_kdconv_bwd_f32(p, p, p, p, cin, p, 0, p, 1, dim, cin, f, p, cin, p, p, 0, p, 1 << 18, _lib.stream_ptr()), "bwd")


# ---- the model --------------------------------------------------------------------------------------------------------------------------

def _seeded_model(dev, seed):
    m = KDNet(num_classes=NC).to(dev)
    copy_into_model(m, seeded_model_state(m, seed))
    return m.train()


def _inputs(B, seed, per_cloud=True):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, 3, 1024)).astype(np.float32)
    sels = [rng.integers(0, 3, size=(B, d) if per_cloud else (d,)) for d in kdnet.DIMS]
    return x, sels


def _recording(monkeypatch):
    """record every level's output of a forward (its autograd node holds the kernel's winner bytes)"""
    rec = []
    inner = kdnet.kdconv

    def wrap(*a, **k):
        out = inner(*a, **k)
        rec.append(out)
        return out
    monkeypatch.setattr(kdnet, "kdconv", wrap)
    return rec


@pytest.mark.parametrize("form", ["B=3 per-cloud packed", "B=1 list"])
def test_model_vs_f64(dev, monkeypatch, form):
    monkeypatch.setattr(kdnet, "_KDCONV", True)
    B = 3 if form.startswith("B=3") else 1
    m = _seeded_model(dev, 31)
    x, sels = _inputs(B, 3, per_cloud=B > 1)
    rec = _recording(monkeypatch)
    if B > 1:
        split = torch.from_numpy(np.concatenate(sels, axis=1).astype(np.int32)).to(dev)          # the packed form [B, 2046]
        logits = m([torch.from_numpy(x).to(dev), split])
    else:
        logits = m([x, [s.astype(np.int64) for s in sels]])                                      # the source's batch: numpy points, ten arrays
    assert logits.shape == (B, NC) and len(rec) == 10
    dec = []
    for out in rec:
        assert type(out.grad_fn).__name__ == "_KDConvBackward"
        dec.append((out.grad_fn.saved_tensors[4].cpu(), (out.detach() > 0).cpu()))
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.named_parameters()}
    ref = kdnet_ref.kdnet(P, torch.from_numpy(x).double(), sels, dec=dec)
    assert_close(_np(logits), _np(ref), BAR, "logits " + form)
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=(B, NC)).astype(np.float32))
    logits.backward(gout.to(dev))
    ref.backward(gout.double())
    bad = []
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        try:
            assert_close(_np(p.grad), _np(P[k].grad), BAR, "d %s %s" % (k, form))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad


def test_torch_op_path_agrees(dev, monkeypatch):
    """PAPC_KDCONV=0: the source's op sequence in torch device ops -- a second, independent implementation of every level.  One train step each."""
    B = 3
    a = _seeded_model(dev, 41)
    b = copy.deepcopy(a)
    x, sels = _inputs(B, 12)
    xd = torch.from_numpy(x).to(dev)
    gout = torch.from_numpy(np.random.default_rng(6).normal(size=(B, NC)).astype(np.float32)).to(dev)
    monkeypatch.setattr(kdnet, "_KDCONV", True)
    la = a([xd, sels])
    la.backward(gout)
    monkeypatch.setattr(kdnet, "_KDCONV", False)
    lb = b([xd, sels])
    lb.backward(gout)
    assert_close(_np(la), _np(lb), BAR, "logits kernel vs torch ops")
    # Gradients: a max-norm bar of 5e-2 only, as test_materialised_concat_agrees (tests/test_gpu_pointnet_seg.py).  The two implementations'
    # activations differ by fp32 rounding, so a ReLU or pair-max decision within rounding of a tie may fall differently, and one flipped
    # decision moves a layer's gradients by about one row's share of their scale -- at B = 3 the last levels have 3 .. 48 rows.  Both are
    # float64-checked: the kernels with pinned decisions in test_model_vs_f64, the torch ops' forward in test_kdconv_kernels_vs_f64.
    bad = []
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        try:
            assert_close(_np(pa.grad), _np(pb.grad), 5e-2, "d %s kernel vs torch ops" % k, elem=float("inf"))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad


def _train_setup(dev, B=8, seed=5):
    from papc_amd.distributed import FlatAdam, FlatParams
    torch.manual_seed(seed)
    m = KDNet(num_classes=NC).to(dev).train()
    flat = FlatParams(m)
    opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)
    x, sels = _inputs(B, seed)
    xd = torch.from_numpy(x).to(dev)
    split = kdnet.pack_split_dims(sels, B, dev)
    y = torch.from_numpy(np.random.default_rng(seed).integers(0, NC, size=B)).to(dev)
    return m, flat, opt, xd, split, y


def _step(m, opt, x, split, y):
    logits = m([x, split])
    loss = H.softmax_cross_entropy(logits, y)
    loss.backward(H.unit_gradient(x.device))
    opt.step_dev(1.0, zero_grad=True, self_tick=True)


def _state(m, flat, opt):
    return [flat.data, flat.grad, opt.m, opt.v, opt.t_dev]


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
    for k in ("kd_fwd_kernel", "kd_fwd3_kernel", "kd_dx_kernel", "kd_dw_kernel", "kd_dw3_kernel"):
        assert any(k in n for n in ours), (k, sorted(names))
    foreign = [n for n in names if not mine(n) and any(s in n.lower() for s in gemmish)]
    assert not foreign, foreign


def test_errors(dev):
    m = KDNet(num_classes=NC).to(dev)
    x, sels = _inputs(2, 1)
    with pytest.raises(_lib.PapcError, match="1000.*1024|1024.*1000"):
        m([torch.zeros(2, 3, 1000, device=dev), sels])
    with pytest.raises(_lib.PapcError):
        m([torch.from_numpy(x), sels])                      # a CPU tensor
    bad = [s.copy() for s in sels]
    bad[4][1, 7] = 3
    with pytest.raises(_lib.PapcError, match="0, 1 or 2"):
        m([x, bad])                                         # a split value of 3 in a numpy list
    with pytest.raises(_lib.PapcError):
        kdnet.kdconv(torch.zeros(64, 32, device=dev, dtype=torch.float64), torch.zeros(32, device=dev, dtype=torch.int32),
                     torch.nn.Conv1d(32, 96, 1).to(dev), 2, 32)


def test_loader_batch_to_loss(dev):
    from papc_amd.datasets import KDClasDataLoader
    rng = np.random.default_rng(21)

    def opener(path):           # a small synthetic ShapeNet-part file (the loader's h5 keys)
        return {"data": rng.normal(size=(2, 1024, 3)).astype(np.float32), "label": rng.integers(0, NC, size=(2, 1))}
    gen = KDClasDataLoader(max_point=1024, batchsize=4, path="shapenet", mode="test", opener=opener)
    batch, label = next(iter(gen()))
    m = _seeded_model(dev, 55)
    logits = m(batch)                                       # the loader's [points, packed split dims] batch, as it comes
    assert logits.shape == (4, NC)
    loss = H.softmax_cross_entropy(logits, torch.from_numpy(label.reshape(-1)).to(dev))
    loss.backward(H.unit_gradient(dev))
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
