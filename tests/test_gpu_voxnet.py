"""GPU tests of the VoxNet classifier (papc_amd.models.VoxNet): the voxconv kernels (csrc/voxconv.hip) against the float64 restatement
(tests/voxnet_ref.py) at edges where tiles are mostly padding, straddle clouds, leave an input plane unused, and at the model's own, the
rejections, the occupancy grid against its host twin, the whole model against float64 with the kernels' decisions pinned, agreement with the
torch-op path (PAPC_VOXNET=0), bit-reproducible and graph-replayable train steps, no foreign GEMM or convolution in a step, the error paths
and a loader batch through to the loss."""
import copy

import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import head as H
from papc_amd import voxnet
from papc_amd.models import VoxNet
from tests import voxnet_ref as R
from tests.util import assert_close

pytestmark = pytest.mark.gpu
BAR = 2e-4          # the project's model-level bar (as tests/test_gpu_kdnet.py)
NC = 10
BB = ("backbone.0.weight", "backbone.0.bias", "backbone.1.weight", "backbone.1.bias", "backbone.3.weight", "backbone.3.bias")


def _np(t):
    return t.detach().double().cpu().numpy()


def _nan(*shape, dev):
    return torch.full(shape, float("nan"), device=dev)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------

def _kernel_fwd(lib, x, P, rmean, rvar, B, E):
    dev, st = x.device, _lib.stream_ptr()
    e1, _, ep = R.edges(E)
    M1, parts = B * e1 ** 3, lib.papc_voxconv_parts(B, E)
    assert parts == -(-M1 // 128)
    y1, part, cst = _nan(M1, 32, dev=dev), _nan(parts, 2, 32, dev=dev), _nan(4, 32, dev=dev)
    wk, wt = _nan(32, 864, dev=dev), _nan(32, 864, dev=dev)
    out, win = _nan(B, 32 * ep ** 3, dev=dev), torch.full((B * ep ** 3, 32), 255, device=dev, dtype=torch.uint8)
    p = lambda k: P[k].data_ptr()                                                                 # noqa: E731
    _lib.check(lib.papc_voxconv1_fwd_f32(x.data_ptr(), p("backbone.0.weight"), p("backbone.0.bias"), B, E, y1.data_ptr(), part.data_ptr(), st), "conv1")
    _lib.check(lib.papc_bn_finalize_f32(part.data_ptr(), parts, M1, 32, p("backbone.1.weight"), p("backbone.1.bias"), R.EPS, voxnet.BN_MOMENTUM,
                                        *_lib.cst_ptrs(cst), rmean.data_ptr(), rvar.data_ptr(), st), "finalize")
    _lib.check(lib.papc_voxconv2_prep_f32(p("backbone.3.weight"), wk.data_ptr(), wt.data_ptr(), st), "prep")
    _lib.check(lib.papc_voxconv2_pool_fwd_f32(y1.data_ptr(), cst[2].data_ptr(), cst[3].data_ptr(), wk.data_ptr(), p("backbone.3.bias"), B, E, out.data_ptr(),
                                              win.data_ptr(), st), "conv2")
    return {"y1": y1, "cst": cst, "wk": wk, "wt": wt, "out": out, "win": win}


def _kernel_bwd(lib, gout, x, f, B, E):
    dev, st = x.device, _lib.stream_ptr()
    e1, _, ep = R.edges(E)
    M1, parts = B * e1 ** 3, lib.papc_voxconv_parts(B, E)
    res = {"gp": _nan(B * ep ** 3, 32, dev=dev), "dz": _nan(M1, 32, dev=dev), "dgamma": _nan(32, dev=dev), "dbeta": _nan(32, dev=dev),
           "dw2": _nan(32, 32, 3, 3, 3, dev=dev), "db2": _nan(32, dev=dev), "dw1": _nan(32, 1, 5, 5, 5, dev=dev), "db1": _nan(32, dev=dev)}
    red, c12 = _nan(parts, 2, 32, dev=dev), _nan(2, 32, dev=dev)
    mean, invstd, scale, shift = _lib.cst_ptrs(f["cst"])
    _lib.check(lib.papc_voxconv2_bwd_dx_f32(gout.data_ptr(), f["win"].data_ptr(), f["wt"].data_ptr(), f["y1"].data_ptr(), mean, invstd, scale, shift, B, E,
                                            res["gp"].data_ptr(), res["dz"].data_ptr(), red.data_ptr(), st), "dx")
    _lib.check(lib.papc_bn_bwd_finalize_f32(red.data_ptr(), parts, M1, 32, res["dgamma"].data_ptr(), res["dbeta"].data_ptr(), c12[0].data_ptr(),
                                            c12[1].data_ptr(), 0, st), "bwd finalize")
    nb = lib.papc_voxconv2_bwd_dw_workspace(B, E)
    ws = torch.full((nb // 4,), float("nan"), device=dev)
    _lib.check(lib.papc_voxconv2_bwd_dw_f32(res["gp"].data_ptr(), f["win"].data_ptr(), f["y1"].data_ptr(), scale, shift, B, E, res["dw2"].data_ptr(),
                                            res["db2"].data_ptr(), 0, ws.data_ptr(), nb, st), "dw2")
    nb = lib.papc_voxconv1_bwd_dw_workspace(B, E)
    ws = torch.full((nb // 4,), float("nan"), device=dev)
    _lib.check(lib.papc_voxconv1_bwd_dw_f32(res["dz"].data_ptr(), f["y1"].data_ptr(), mean, invstd, scale, c12[0].data_ptr(), c12[1].data_ptr(), x.data_ptr(),
                                            B, E, res["dw1"].data_ptr(), res["db1"].data_ptr(), 0, ws.data_ptr(), nb, st), "dw1")
    return res


def _sign1(f):
    """the sign the kernels take: scale * y1 + shift > 0 of their own stored rows and constants, in float64 (the product is exact there)"""
    return ((f["cst"][2].double() * f["y1"].double() + f["cst"][3].double()) > 0).cpu()


@pytest.mark.parametrize("E", [12, 15, 16, 32])
@pytest.mark.parametrize("B", [1, 3])
def test_voxconv_kernels_vs_f64(dev, E, B):
    lib = _lib.load()
    assert voxnet.kernel_ok(E)
    tag = "E=%d B=%d" % (E, B)
    e1, _, ep = R.edges(E)
    g = torch.Generator().manual_seed(17 * E + B)
    x64 = torch.randn(B, 1, E, E, E, generator=g, dtype=torch.float64).float().double()           # randn, not 0/1: a wrong tap lands on a wrong value
    gout64 = torch.randn(B, 32 * ep ** 3, generator=g, dtype=torch.float64).float().double()
    P64 = {k: v.float().double() for k, v in R.params(E, 5 + E).items()}
    P = {k: P64[k].float().to(dev) for k in BB}
    x, gout = x64.float().to(dev), gout64.float().to(dev)
    rmean, rvar = torch.zeros(32, device=dev), torch.ones(32, device=dev)
    f = _kernel_fwd(lib, x, P, rmean, rvar, B, E)
    # forward against the reference's own decisions
    ref = R.backbone_closed(P64, x64)
    assert_close(_np(f["y1"]), _np(ref["y1"]), BAR, "y1 " + tag)
    assert_close(_np(f["cst"][0]), _np(ref["mean"]), BAR, "mean " + tag)
    assert_close(_np(f["cst"][1]), _np(1.0 / torch.sqrt(ref["var"] + R.EPS)), BAR, "1/sigma " + tag)
    assert_close(_np(rmean), _np(0.1 * ref["mean"]), BAR, "running mean " + tag)                  # 0.9 * 0 + 0.1 * batch
    assert_close(_np(rvar), _np(0.9 + 0.1 * ref["var"]), BAR, "running var (biased) " + tag)
    assert_close(_np(f["out"]), _np(ref["flat"]), BAR, "pooled, flatten order " + tag)
    assert int(f["win"].max()) <= 7
    # backward against float64 routed by the kernels' own decisions
    Pg = {k: v.clone().requires_grad_(True) for k, v in P64.items()}
    pin = R.backbone_closed(Pg, x64, win=f["win"].cpu(), sign1=_sign1(f))
    pin["flat"].backward(gout64)
    res = _kernel_bwd(lib, gout, x, f, B, E)
    assert_close(_np(res["dz"]), _np(pin["t"].grad), BAR, "dz " + tag)
    for k, name in (("dgamma", "backbone.1.weight"), ("dbeta", "backbone.1.bias"), ("dw2", "backbone.3.weight"), ("db2", "backbone.3.bias"),
                    ("dw1", "backbone.0.weight")):
        assert_close(_np(res[k]), _np(Pg[name].grad), BAR, "%s %s" % (k, tag))
    assert bool((res["db1"] == 0).all()), "conv1.bias under a train-mode norm: exactly 0 " + tag
    # two identical calls: bit-identical (no atomics, fixed-order folds)
    f2 = _kernel_fwd(lib, x, P, torch.zeros(32, device=dev), torch.ones(32, device=dev), B, E)
    for k in f:
        assert torch.equal(f[k], f2[k]), k + " " + tag
    res2 = _kernel_bwd(lib, gout, x, f, B, E)
    for k in res:
        assert torch.equal(res[k], res2[k]), k + " " + tag
    # the torch-op path (PAPC_VOXNET=0): the same forward
    m = VoxNet(num_classes=NC).to(dev).train()
    with torch.no_grad():
        for k in BB:
            dict(m.named_parameters())[k].copy_(P[k])
    assert_close(_np(voxnet._backbone_torch(x, m.backbone[0], m.backbone[1], m.backbone[3], True)), _np(ref["flat"]), BAR, "torch-op pooled " + tag)
    assert_close(_np(m.backbone[1].running_var), _np(0.9 + 0.1 * ref["var"]), BAR, "torch-op running var " + tag)


def test_voxconv_rejects_other_edges(dev):
    lib = _lib.load()
    t = torch.zeros(1 << 16, device=dev)
    p, st = t.data_ptr(), _lib.stream_ptr()
    for E in (13, 10, 34):
        assert not voxnet.kernel_ok(E)
        calls = (lambda: lib.papc_voxconv1_fwd_f32(p, p, p, 1, E, p, p, st),
                 lambda: lib.papc_voxconv2_pool_fwd_f32(p, p, p, p, p, 1, E, p, p, st),
                 lambda: lib.papc_voxconv2_bwd_dx_f32(p, p, p, p, p, p, p, p, 1, E, p, p, p, st),
                 lambda: lib.papc_voxconv2_bwd_dw_f32(p, p, p, p, p, 1, E, p, p, 0, p, 1 << 18, st),
                 lambda: lib.papc_voxconv1_bwd_dw_f32(p, p, p, p, p, p, p, p, 1, E, p, p, 0, p, 1 << 18, st))
        for call in calls:
            assert call() == -2                                                                   # PAPC_E_UNSUPPORTED
            with pytest.raises(_lib.PapcError, match="E=%d" % E):
                _lib.check(call(), "voxconv")


def test_occupancy_grid_equals_host_twin(dev):
    pts = R.occupancy_fixture()
    for edge in (32, 12):
        got = voxnet.occupancy_grid(torch.from_numpy(pts).to(dev), edge)
        assert got.shape == (2, 1, edge, edge, edge)
        assert np.array_equal(got.cpu().numpy(), voxnet.occupancy_grid_np(pts, edge))
    bad = pts.copy()
    bad[1, 7, 1] = np.float32(1.25)
    bad[0, 9, 0] = np.float32(-3.0)
    with pytest.raises(_lib.PapcError, match="2 points"):
        voxnet.occupancy_grid(torch.from_numpy(bad).to(dev))
    with pytest.raises(_lib.PapcError):
        voxnet.occupancy_grid(torch.from_numpy(pts))                                              # a CPU tensor


# ---- the model --------------------------------------------------------------------------------------------------------------------------

def _seeded_model(dev, seed):
    """the reference's seeded parameters at the model's edge (tests.util.seeded_model_state does not know backbone.1 as a norm)"""
    m = VoxNet(num_classes=NC).to(dev)
    P64 = {k: v.float().double() for k, v in R.params(32, seed, NC).items()}
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(P64[k].float())
    return m.train(), P64


def _grid(B, seed, dev):
    """an occupancy input from ~1024 random points per cloud"""
    pts = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(B, 1024, 3)).astype(np.float32)
    return voxnet.occupancy_grid(torch.from_numpy(pts).to(dev))


def _recording(monkeypatch):
    rec = {}
    bb, ld = voxnet.voxconv_backbone, voxnet.leaky_dropout

    def wrap_bb(*a, **k):
        rec["bb"] = bb(*a, **k)
        return rec["bb"]

    def wrap_ld(*a, **k):
        rec["ld"] = ld(*a, **k)
        return rec["ld"]
    monkeypatch.setattr(voxnet, "voxconv_backbone", wrap_bb)
    monkeypatch.setattr(voxnet, "leaky_dropout", wrap_ld)
    return rec


def test_model_vs_f64(dev, monkeypatch):
    monkeypatch.setattr(voxnet, "_VOXNET", True)
    B = 3
    m, P64 = _seeded_model(dev, 31)
    x = _grid(B, 3, dev)
    assert 0 < float(x.sum()) <= B * 1024 and set(np.unique(x.cpu().numpy())) == {0.0, 1.0}
    rec = _recording(monkeypatch)
    logits = m(x)
    assert logits.shape == (B, NC)
    assert type(rec["bb"].grad_fn).__name__ == "_VoxBackboneBackward" and type(rec["ld"].grad_fn).__name__ == "_LeakyDropoutBackward"
    _, y1, cst, _, win = rec["bb"].grad_fn.saved_tensors
    h, keep = rec["ld"].grad_fn.saved_tensors
    assert keep is not None and 0.6 < float(keep.float().mean()) < 0.95                           # Dropout(0.2)
    dec = (win.cpu(), _sign1({"cst": cst, "y1": y1}), (h > 0).cpu(), keep.cpu())
    P = {k: v.clone().requires_grad_(True) for k, v in P64.items()}
    ref, bb = R.closed(P, x.double().cpu(), dec=dec)
    assert_close(_np(logits), _np(ref), BAR, "logits")
    gout = torch.from_numpy(np.random.default_rng(5).normal(size=(B, NC)).astype(np.float32))
    logits.backward(gout.to(dev))
    ref.backward(gout.double())
    bad = []
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        if k == "backbone.0.bias":
            assert bool((p.grad == 0).all()), "conv1.bias under a train-mode norm: exactly 0"
            continue
        try:
            assert_close(_np(p.grad), _np(P[k].grad), BAR, "d " + k)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad
    # one plain SGD step, then eval mode: the norm on the running statistics the train forward left, no dropout, nothing updated
    with torch.no_grad():
        for p in m.parameters():
            p.sub_(0.01 * p.grad)
    bn = m.backbone[1]
    assert_close(_np(bn.running_mean), _np(0.1 * bb["mean"]), BAR, "running mean")
    assert_close(_np(bn.running_var), _np(0.9 + 0.1 * bb["var"]), BAR, "running var")
    m.eval()
    before = (bn.running_mean.clone(), bn.running_var.clone())
    with torch.no_grad():
        ev = m(x)
        assert torch.equal(ev, m(x))
    assert torch.equal(before[0], bn.running_mean) and torch.equal(before[1], bn.running_var)
    Pe = {k: v.detach().double().cpu() for k, v in m.named_parameters()}
    ref_ev, _ = R.closed(Pe, x.double().cpu(), stats=(bn.running_mean.double().cpu(), bn.running_var.double().cpu()))
    assert_close(_np(ev), _np(ref_ev), BAR, "eval logits")


def test_torch_op_path_agrees(dev, monkeypatch):
    """PAPC_VOXNET=0: the backbone in torch device ops -- a second, independent implementation.  One train step each (the same dropout mask:
    both models draw it from the same seed and counter)."""
    B = 3
    a, _ = _seeded_model(dev, 41)
    b = copy.deepcopy(a)
    x = _grid(B, 12, dev)
    gout = torch.from_numpy(np.random.default_rng(6).normal(size=(B, NC)).astype(np.float32)).to(dev)
    monkeypatch.setattr(voxnet, "_VOXNET", True)
    la = a(x)
    la.backward(gout)
    monkeypatch.setattr(voxnet, "_VOXNET", False)
    lb = b(x)
    lb.backward(gout)
    assert type(la.grad_fn).__name__ == type(lb.grad_fn).__name__                                 # (the head is the same nodes on both paths)
    assert_close(_np(la), _np(lb), BAR, "logits kernel vs torch ops")
    # Gradients: a max-norm bar of 5e-2 only, as tests/test_gpu_kdnet.py::test_torch_op_path_agrees and for its reason: the two implementations'
    # activations differ by fp32 rounding, so a LeakyReLU sign or a pool winner within rounding of a tie may fall differently.  Both are
    # float64-checked: the kernels with pinned decisions in test_model_vs_f64, the torch ops' forward in test_voxconv_kernels_vs_f64.
    bad = []
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if k == "backbone.0.bias":
            # a bias under a train-mode norm: the kernels write the exact 0, autograd leaves rounding noise around it -- read at the same bar on
            # the scale of the gradient of the weight it belongs to (a ratio of two zeros says nothing)
            assert bool((pa.grad == 0).all())
            assert float(pb.grad.abs().max()) <= 5e-2 * float(b.backbone[0].weight.grad.abs().max()), "d backbone.0.bias of the torch-op path"
            continue
        try:
            assert_close(_np(pa.grad), _np(pb.grad), 5e-2, "d %s kernel vs torch ops" % k, elem=float("inf"))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad


def _train_setup(dev, B=8, seed=5):
    from papc_amd.distributed import FlatAdam, FlatParams
    torch.manual_seed(seed)
    m = VoxNet(num_classes=NC).to(dev).train()
    flat = FlatParams(m)
    opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)
    x = _grid(B, seed, dev)
    y = torch.from_numpy(np.random.default_rng(seed).integers(0, NC, size=B)).to(dev)
    return m, flat, opt, x, y


def _step(m, opt, x, y):
    logits = m(x)
    loss = H.softmax_cross_entropy(logits, y)
    loss.backward(H.unit_gradient(x.device))
    opt.step_dev(1.0, zero_grad=True, self_tick=True)


def _state(m, flat, opt):
    bn = m.backbone[1]
    return [flat.data, flat.grad, opt.m, opt.v, opt.t_dev, bn.running_mean, bn.running_var, m.head_spec.rng_state]


def test_train_step_bit_reproducible_and_graph_replay_equal(dev, monkeypatch):
    monkeypatch.setattr(voxnet, "_VOXNET", True)
    m, flat, opt, x, y = _train_setup(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                     # warm-up (eager, side stream) before the capture
            _step(m, opt, x, y)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    snap = [t.clone() for t in _state(m, flat, opt)]
    assert int(snap[-1][1]) == 2               # the dropout counter: one draw per step

    def restore():
        with torch.no_grad():
            for t, v in zip(_state(m, flat, opt), snap):
                t.copy_(v)
        torch.cuda.synchronize()

    _step(m, opt, x, y)
    torch.cuda.synchronize()
    eager1 = [t.clone() for t in _state(m, flat, opt)]
    restore()
    _step(m, opt, x, y)
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
            _step(m, opt, x, y)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    restore()
    g.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(eager1, _state(m, flat, opt))):
        assert torch.equal(a, b), "graph replay differs from the eager step (state tensor %d)" % i


def test_train_step_runs_no_foreign_gemm_or_convolution(dev, monkeypatch):
    from torch.profiler import ProfilerActivity, profile
    monkeypatch.setattr(voxnet, "_VOXNET", True)
    m, flat, opt, x, y = _train_setup(dev)
    _step(m, opt, x, y)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        _step(m, opt, x, y)
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    gemmish = ("cijk", "gemm", "gemv", "bmm", "matmul", "rocblas", "hipblas", "tensile", "mfma", "conv", "miopen", "im2col")
    mine = lambda n: "papc::" in n.split("(")[0] or n.startswith("_ZN4papc")      # (demangled or not)
    ours = [n for n in names if mine(n)]
    for k in ("vox_conv1_fwd_kernel", "vox_w2_prep_kernel", "vox_conv2_pool_kernel", "vox_gp_kernel", "vox_db2_kernel", "vox_conv2_dx_kernel",
              "vox_conv2_dw_kernel", "vox_conv1_dw_kernel", "vox_leaky_drop_fwd_kernel", "vox_rng_bump_kernel", "vox_leaky_drop_bwd_kernel"):
        assert any(k in n for n in ours), (k, sorted(names))
    foreign = [n for n in names if not mine(n) and any(s in n.lower() for s in gemmish)]
    assert not foreign, foreign


def test_errors(dev):
    m = VoxNet(num_classes=NC).to(dev)
    with pytest.raises(_lib.PapcError):
        m(torch.zeros(2, 1, 32, 32, 32))                                                          # a CPU tensor
    with pytest.raises(_lib.PapcError, match=r"\[B, 1, 32, 32, 32\].*30"):
        m(torch.zeros(2, 1, 30, 30, 30, device=dev))
    with pytest.raises(_lib.PapcError, match="float32"):
        m(torch.zeros(2, 1, 32, 32, 32, device=dev, dtype=torch.float64))
    with pytest.raises(_lib.PapcError, match=r"\[B, 1, 32, 32, 32\]"):
        m(torch.zeros(2, 2, 32, 32, 32, device=dev))
    b = m.backbone
    with pytest.raises(_lib.PapcError):
        voxnet.voxconv_backbone(torch.zeros(2, 1, 16, 16, 16), b[0], b[1], b[3], True)            # a CPU tensor
    with pytest.raises(_lib.PapcError, match="float32"):
        voxnet.voxconv_backbone(torch.zeros(2, 1, 16, 16, 16, device=dev, dtype=torch.float64), b[0], b[1], b[3], True)
    with pytest.raises(_lib.PapcError, match=r"\[B, 1, E, E, E\]"):
        voxnet.voxconv_backbone(torch.zeros(2, 2, 16, 16, 16, device=dev), b[0], b[1], b[3], True)
    with pytest.raises(_lib.PapcError, match=r"\[B, 1, E, E, E\]"):
        voxnet.voxconv_backbone(torch.zeros(2, 1, 16, 16, 12, device=dev), b[0], b[1], b[3], True)


def test_loader_batch_to_loss(dev, tmp_path):
    from papc_amd import datasets as D
    rng = np.random.default_rng(21)
    with open(tmp_path / "test.txt", "w") as f:
        for i in range(5):
            np.save(tmp_path / ("g%d.npy" % i), voxnet.occupancy_grid_np(rng.uniform(-1, 1, size=(1, 256, 3)).astype(np.float32))[0, 0])
            f.write("g%d.npy %s\n" % (i, D.categoryList[i]))
    gen = D.DataLoader("voxnet", 1024, 4, str(tmp_path), "clas", "test")
    x, y = next(D.device_batches(gen, dev))
    assert x.shape == (4, 1, 32, 32, 32) and y.shape == (4,) and y.tolist() == [0, 1, 2, 3]
    m, _ = _seeded_model(dev, 55)
    loss = H.softmax_cross_entropy(m(x), y)
    loss.backward(H.unit_gradient(dev))
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
