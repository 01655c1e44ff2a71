"""GPU tests of the T-Net PointNet classifier (papc_amd.models.PointNet_Clas, pointnet_Conv1D.py:4-104): the per-cloud transform kernels
(csrc/cloud_transform.hip) and the T-Net FC blocks on the head kernels against float64, the whole model against a float64 restatement
(tests/pointnet_ref.py) in train and eval mode, bit-reproducible and graph-replayable train steps, and no library GEMM in a step."""
import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import head as H
from papc_amd.models import PointNet_Basic_Clas, PointNet_Clas
from papc_amd.transform import tnet_fc, transform_points, transform_rows
from tests import pointnet_ref
from tests.util import assert_close, copy_into_model, kernel_decisions, seeded_model_state

pytestmark = pytest.mark.gpu
BAR = 2e-4          # the project's model-level bar


def _np(t):
    return t.detach().double().cpu().numpy()


def _transform_case(dev, C, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    T = torch.randn(B, C, C, generator=g) / np.sqrt(C)
    if C == 3:
        x = torch.randn(B, 3, N, generator=g)                  # planar model input, read through strides
        x_pts = x.transpose(1, 2)
    else:
        x = torch.randn(B * N, C, generator=g)                 # mlp_1's rows
        x_pts = x.view(B, N, C)
    gy = torch.randn(B, N, C, generator=g)
    return x.to(dev), T.to(dev), gy.to(dev), x_pts.double(), T.double(), gy.double()


@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("N", [1000, 1024, 2048])
@pytest.mark.parametrize("B", [1, 32, 33])
def test_transform_kernels_vs_f64_bmm(dev, C, B, N):
    x, T, gy, x64, T64, gy64 = _transform_case(dev, C, B, N, 100 * C + B + N)
    x.requires_grad_(True)
    T.requires_grad_(True)
    y = transform_points(x, T) if C == 3 else transform_rows(x, T, N)
    ref = torch.bmm(x64, T64)                                               # [B, N, C]
    assert_close(_np(y).reshape(B, N, C), ref.numpy(), BAR, "transform C=%d forward" % C)
    y.backward(gy.view(y.shape))
    dx_ref = torch.bmm(gy64, T64.transpose(1, 2))                           # dY T^T
    dT_ref = torch.bmm(x64.transpose(1, 2), gy64)                           # X^T dY
    dx = x.grad if C == 64 else x.grad.transpose(1, 2)
    assert_close(_np(dx).reshape(B, N, C), dx_ref.numpy(), BAR, "transform C=%d dX" % C)
    assert_close(_np(T.grad), dT_ref.numpy(), BAR, "transform C=%d dT" % C)
    # a second backward of the same graph: bit-identical (no atomics; fixed-order fold)
    dx1, dT1 = x.grad.clone(), T.grad.clone()
    x.grad, T.grad = None, None
    y2 = transform_points(x, T) if C == 3 else transform_rows(x, T, N)
    assert torch.equal(y2, y)
    y2.backward(gy.view(y.shape))
    assert torch.equal(x.grad, dx1) and torch.equal(T.grad, dT1)
    # accumulate flag of the raw entry point: dX added to what the buffer holds
    lib = _lib.load()
    base = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    acc = base.clone()
    dT = torch.empty(B, C, C, device=dev)
    nb = lib.papc_cloud_transform_bwd_workspace(B, N, C)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    xs = (3 * N, 1, N) if C == 3 else (N * C, C, 1)
    _lib.check(lib.papc_cloud_transform_bwd_f32(x.data_ptr(), xs[0], xs[1], xs[2], T.data_ptr(), C * C, gy.data_ptr(), B, N, C, acc.data_ptr(),
                                                xs[0], xs[1], xs[2], 1, dT.data_ptr(), ws.data_ptr(), nb, _lib.stream_ptr()), "bwd")
    torch.cuda.synchronize()
    acc_ref = base.double().cpu() + (dx_ref.transpose(1, 2) if C == 3 else dx_ref.reshape(B * N, C))
    assert_close(_np(acc), acc_ref.numpy(), BAR, "transform C=%d dX accumulated" % C)
    assert torch.equal(dT, dT1)


def test_transform_rejects_other_widths(dev):
    x = torch.zeros(2 * 8, 5, device=dev)
    with pytest.raises(_lib.PapcError, match="C=5"):
        transform_rows(x, torch.zeros(2, 5, 5, device=dev), 8)


def _fc(widths, seed, dev):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(widths[0], widths[1]), torch.nn.ReLU(), torch.nn.Linear(widths[1], widths[2]), torch.nn.ReLU(),
                               torch.nn.Linear(widths[2], widths[3])).to(dev)


@pytest.mark.parametrize("cout", [9, 4096])
def test_tnet_fc_on_head_kernels_vs_f64(dev, cout):
    B = 32
    fc = _fc([1024, 512, 256, cout], 11 + cout, dev)
    g = torch.Generator().manual_seed(cout)
    x = torch.relu(torch.randn(B, 1024, generator=g)).to(dev).requires_grad_(True)
    gout = torch.randn(B, cout, generator=g).to(dev)
    out = tnet_fc(H.HeadSpec(), x, fc)
    assert out.shape == (B, cout)
    P = {"f.%d.%s" % (i, n): getattr(fc[i], n).detach().double().cpu().requires_grad_(True) for i in (0, 2, 4) for n in ("weight", "bias")}
    x64 = x.detach().double().cpu().requires_grad_(True)
    ref = pointnet_ref.fc_block(P, "f", x64, [0, 2, 4])
    assert_close(_np(out), _np(ref), BAR, "T-Net FC %d forward" % cout)
    out.backward(gout)
    ref.backward(gout.double().cpu())
    assert_close(_np(x.grad), _np(x64.grad), BAR, "T-Net FC %d dX" % cout)
    for i in (0, 2, 4):
        for n in ("weight", "bias"):
            assert_close(_np(getattr(fc[i], n).grad), _np(P["f.%d.%s" % (i, n)].grad), BAR, "T-Net FC %d d%s.%s" % (cout, i, n))


def test_plain_usable_unchanged_for_pointnet_basic(dev):
    """The 9-wide T-Net layer is padded inside its own node: the head gate of PointNet-Basic answers exactly as before (10 classes: the module
    chain, 16 classes: the head kernels)."""
    feat = torch.zeros(8, 1024, device=dev)
    for nc, want in ((10, False), (16, True)):
        m = PointNet_Basic_Clas(num_classes=nc).to(dev)
        assert H.plain_usable(feat, m.fc[0], m.fc[2], m.fc[5], True) is want
        assert H.plain_usable(feat, m.fc[0], m.fc[2], m.fc[5], False) is want


def _seeded_model(dev, seed, N=1024):
    m = PointNet_Clas(16, N).to(dev)
    st = seeded_model_state(m, seed)
    for k in st:              # the T-Net FC blocks as the source starts them (input_fc: zero weight, identity bias), perturbed so that
        if k.startswith(("input_fc.4", "feature_fc.4")):      # every layer of the chain carries a gradient
            st[k] = st[k] * 0.05
    st["input_fc.4.bias"] = (np.eye(3).reshape(-1) + st["input_fc.4.bias"]).astype(np.float32)
    st["feature_fc.4.bias"] = (np.eye(64).reshape(-1) + st["feature_fc.4.bias"]).astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    for name, mod in m.named_modules():         # (the norms: seeded_model_state knows them by "bn" / "norm" in their names)
        if isinstance(mod, torch.nn.BatchNorm1d):
            c = mod.num_features
            st[name + ".weight"] = (rng.uniform(0.5, 1.5, size=c) * rng.choice([1.0, 1.0, 1.0, -1.0], size=c)).astype(np.float32)
            st[name + ".bias"] = (rng.normal(size=c) * 0.2).astype(np.float32)
    copy_into_model(m, st)
    return m


def _recording(monkeypatch):
    """record the stack and FC-block outputs of a forward (their autograd nodes hold the kernels' decisions)"""
    import papc_amd.models as M
    import papc_amd.transform as T
    rec = {"stacks": [], "tnet": [], "head": []}
    smm, tf, ph = M.shared_mlp_max, T.tnet_fc, H.plain_head

    def smm_rec(*a, **k):
        out = smm(*a, **k)
        rec["stacks"].append(out)
        return out

    def tf_rec(*a, **k):
        out = tf(*a, **k)
        rec["tnet"].append(out)
        return out

    def ph_rec(*a, **k):
        out = ph(*a, **k)
        rec["head"].append(out)
        return out
    monkeypatch.setattr(M, "shared_mlp_max", smm_rec)
    monkeypatch.setattr(T, "tnet_fc", tf_rec)
    monkeypatch.setattr(H, "plain_head", ph_rec)
    return rec


def _head_masks(out):
    saved = out.grad_fn.saved_tensors                 # _HeadPlain: (x0, w1, w2, w3, relu1 out, dropout(relu2) out)
    return saved[4] > 0, saved[5] > 0


def test_model_train_mode_vs_f64(dev, monkeypatch):
    B, N = 8, 1024
    m = _seeded_model(dev, 31).train()
    m._spec("_head_spec").export_masks = True
    rec = _recording(monkeypatch)
    x = torch.from_numpy(np.random.default_rng(3).normal(size=(B, 3, N)).astype(np.float32)).to(dev)
    gout = torch.from_numpy(np.random.default_rng(4).normal(size=(B, 16)).astype(np.float32)).to(dev)
    logits = m(x)
    assert len(rec["stacks"]) == 4 and len(rec["tnet"]) == 2 and len(rec["head"]) == 2   # (head: feature_fc's block, then the classifier)
    names = ["input_transform_net", "mlp_1", "feature_transform_net", "mlp_2"]
    dec = {}
    for nm, out in zip(names, rec["stacks"]):
        argmax, alive, masks = kernel_decisions(out)
        dec[nm] = (argmax.cpu() if argmax is not None else None, alive.cpu(), [None if mk is None else mk.cpu() for mk in masks])
    for nm, out in zip(["input_fc", "feature_fc"], rec["tnet"]):
        m1, m2 = _head_masks(out)
        dec[nm] = (m1.cpu(), m2.cpu(), None)
    m1, m2 = _head_masks(logits)
    dec["fc"] = (m1.cpu(), m2.cpu(), m._head_spec.masks[0].bool().cpu())
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.named_parameters()}
    ref = pointnet_ref.pointnet_clas(P, x.double().cpu(), train=True, dec=dec)
    assert_close(_np(logits), _np(ref), BAR, "PointNet_Clas train logits")
    logits.backward(gout)
    ref.backward(gout.double().cpu())
    bad = []
    for k, p in m.named_parameters():
        g, r = p.grad, P[k].grad
        assert g is not None, k
        conv_bias = k.endswith(".bias") and any(k.startswith(s) for s in names) and int(k.split(".")[1]) % 3 == 0
        if conv_bias:      # a conv bias in front of a train-mode BatchNorm: its gradient is ~0 on both sides
            wk = k[:-4] + "weight"
            assert float(g.abs().max()) <= 1e-4 * float(P[wk].grad.abs().max()), k
            continue
        try:
            assert_close(_np(g), _np(r), BAR, "d " + k)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad


def test_model_eval_mode_vs_f64(dev):
    B, N = 8, 1024
    m = _seeded_model(dev, 37)
    rng = np.random.default_rng(9)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(torch.from_numpy(rng.normal(size=mod.num_features).astype(np.float32) * 0.1))
                mod.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, size=mod.num_features).astype(np.float32)))
    m.eval()
    x = torch.from_numpy(rng.normal(size=(B, 3, N)).astype(np.float32)).to(dev)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        logits = m(x)
    P = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    ref = pointnet_ref.pointnet_clas(P, x.double().cpu(), train=False)
    assert_close(_np(logits), _np(ref), BAR, "PointNet_Clas eval logits")
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k           # eval leaves the running statistics untouched


def _train_setup(dev, B=32, N=1024, seed=5):
    from papc_amd.distributed import FlatAdam, FlatParams
    torch.manual_seed(seed)
    m = PointNet_Clas(16, N).to(dev).train()
    flat = FlatParams(m)
    opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.normal(size=(B, 3, N)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, 16, size=B)).to(dev)
    return m, flat, opt, x, y


def _step(m, opt, x, y):
    loss = H.softmax_cross_entropy(m(x), y)
    loss.backward(H.unit_gradient(x.device))
    opt.step_dev(1.0, zero_grad=True, self_tick=True)


def _state(m, flat, opt):
    st = [flat.data, flat.grad, opt.m, opt.v, opt.t_dev] + [b for b in m.buffers()]
    st += [s.rng_state for s in (m.__dict__.get(n) for n in ("_spec_input_fc", "_spec_feature_fc", "_head_spec")) if s is not None and s.rng_state is not None]
    return st


def test_train_step_bit_reproducible_and_graph_replay_equal(dev):
    m, flat, opt, x, y = _train_setup(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                     # warm-up (eager, side stream) before the capture
            _step(m, opt, x, y)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    snap = [t.clone() for t in _state(m, flat, opt)]

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


def test_train_step_runs_no_library_gemm(dev):
    from torch.profiler import ProfilerActivity, profile
    m, flat, opt, x, y = _train_setup(dev)
    _step(m, opt, x, y)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        _step(m, opt, x, y)
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    gemmish = ("cijk", "gemm", "gemv", "bmm", "matmul", "rocblas", "hipblas", "tensile", "mfma")
    mine = lambda n: "papc::" in n.split("(")[0] or n.startswith("_ZN4papc")      # (demangled or not)
    ours = [n for n in names if mine(n)]
    assert any("ct_bwd64" in n for n in ours) and any("ct_fwd3" in n for n in ours), sorted(names)
    foreign = [n for n in names if not mine(n) and any(s in n.lower() for s in gemmish)]
    assert not foreign, foreign


def test_errors(dev):
    m = PointNet_Clas(16, 1024).to(dev)
    with pytest.raises(_lib.PapcError, match="1000.*1024|1024.*1000"):
        m(torch.zeros(2, 3, 1000, device=dev))
    with pytest.raises(_lib.PapcError):
        m.cpu()(torch.zeros(2, 3, 1024))
