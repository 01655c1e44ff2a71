"""GPU tests of the PointNet part segmenters (papc_amd.models.PointNet_Seg / PointNet_Basic_Seg): the concat-conv kernels
(csrc/cloud_concat.hip) against float64 on the materialised concat, the whole models against a float64 restatement
(tests/pointnet_seg_ref.py) in train and eval mode, agreement with the materialised path (PAPC_SEG_CONCAT=0), bit-reproducible and
graph-replayable train steps, no library GEMM in a step, the error paths and a loader batch through to the loss."""
import copy

import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import head as H
from papc_amd.models import PointNet_Basic_Seg, PointNet_Seg
from tests import concat_cases, pointnet_seg_ref
from tests.util import assert_close, copy_into_model, kernel_decisions, seeded_model_state

pytestmark = pytest.mark.gpu
BAR = 2e-4          # the project's model-level bar (as tests/test_gpu_pointnet.py)
NC = 50


def _np(t):
    return t.detach().double().cpu().numpy()


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cg", [64, 1024])
@pytest.mark.parametrize("N", [1000, 1024, 2048])
@pytest.mark.parametrize("B", [1, 32, 33])
def test_concat_conv_kernels_vs_f64(dev, B, N, cg):
    from papc_amd.segment import FAMILY
    concat_cases.check_kernels_vs_f64(FAMILY, dev, B, N, 64, cg, 512, 1000 * B + N + cg, BAR, "B=%d N=%d Cg=%d" % (B, N, cg))


def test_concat_conv_rejects_other_shapes(dev):
    lib = _lib.load()
    t = torch.zeros(4 * 8, 1024 + 64, device=dev)
    p = t.data_ptr()
    for cp, cg, cout, what in ((64, 96, 512, "Cg=96"), (64, 2048, 512, "Cg=2048"), (32, 64, 512, "Cp=32"), (64, 64, 256, "Cout=256")):
        with pytest.raises(_lib.PapcError, match=what):
            _lib.check(lib.papc_cloud_concat_conv_f32(p, 64, p, p, None, 4, 8, cp, cg, cout, p, p, None, _lib.stream_ptr()), "fwd")
        with pytest.raises(_lib.PapcError, match=what):
            _lib.check(lib.papc_cloud_concat_conv_bwd_f32(p, p, p, p, p, p, p, p, p, 64, p, p, 4, 8, cp, cg, cout, p, 64, 0, p, p, p, None, p, 1 << 20,
                                                          _lib.stream_ptr()), "bwd")


# ---- the models -------------------------------------------------------------------------------------------------------------------------

STACKS = {"pointnet": ["input_transform_net", "mlp_1", "feature_transform_net", "mlp_2", "seg1"],
          "pointnet_basic": ["mlp_1", "mlp_2", "seg1"]}
CONV_SEQS = {"pointnet": ("input_transform_net", "mlp_1", "feature_transform_net", "mlp_2", "seg_net"),
             "pointnet_basic": ("pointnet_bacic.mlp_1", "pointnet_bacic.mlp_2", "seg_net")}


def _make(kind, N=1024):
    return PointNet_Seg(NC, N) if kind == "pointnet" else PointNet_Basic_Seg(NC, N)


def _ref(kind):
    return pointnet_seg_ref.pointnet_seg if kind == "pointnet" else pointnet_seg_ref.pointnet_basic_seg


def _seeded_model(dev, kind, seed, N=1024):
    m = _make(kind, N).to(dev)
    st = seeded_model_state(m, seed)
    if kind == "pointnet":      # the T-Net FC blocks as the source starts them, perturbed so that every layer carries a gradient
        for k in st:
            if k.startswith(("input_fc.4", "feature_fc.4")):
                st[k] = st[k] * 0.05
        st["input_fc.4.bias"] = (np.eye(3).reshape(-1) + st["input_fc.4.bias"]).astype(np.float32)
        st["feature_fc.4.bias"] = (np.eye(64).reshape(-1) + st["feature_fc.4.bias"]).astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    for name, mod in m.named_modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            c = mod.num_features
            st[name + ".weight"] = (rng.uniform(0.5, 1.5, size=c) * rng.choice([1.0, 1.0, 1.0, -1.0], size=c)).astype(np.float32)
            st[name + ".bias"] = (rng.normal(size=c) * 0.2).astype(np.float32)
    copy_into_model(m, st)
    return m


def _recording(monkeypatch):
    """record the stack, T-Net FC and concat-layer outputs of a forward (their autograd nodes hold the kernels' decisions)"""
    import papc_amd.models as M
    import papc_amd.segment as S
    import papc_amd.transform as T
    rec = {"stacks": [], "tnet": [], "concat": []}

    def wrap(fn, key):
        def inner(*a, **k):
            out = fn(*a, **k)
            rec[key].append(out)
            return out
        return inner
    monkeypatch.setattr(M, "shared_mlp_max", wrap(M.shared_mlp_max, "stacks"))
    monkeypatch.setattr(T, "tnet_fc", wrap(T.tnet_fc, "tnet"))
    monkeypatch.setattr(S, "cloud_concat_bn_relu", wrap(S.cloud_concat_bn_relu, "concat"))
    return rec


def _decisions(kind, rec):
    dec = {}
    assert len(rec["stacks"]) == len(STACKS[kind]) and len(rec["concat"]) == 1
    for nm, out in zip(STACKS[kind], rec["stacks"]):
        argmax, alive, masks = kernel_decisions(out)
        dec[nm] = (argmax.cpu() if argmax is not None else None, alive.cpu(), [None if mk is None else mk.cpu() for mk in masks])
    for nm, out in zip(["input_fc", "feature_fc"], rec["tnet"]):
        saved = out.grad_fn.saved_tensors             # _HeadPlain: (x0, w1, w2, w3, relu1 out, relu2 out)
        dec[nm] = ((saved[4] > 0).cpu(), (saved[5] > 0).cpu(), None)
    dec["seg0"] = (None, (rec["concat"][0].detach() > 0).cpu(), None)
    return dec


def _is_conv_bias_before_bn(kind, k):
    """parameters whose exact gradient is ~0: a conv bias in front of a train-mode BatchNorm, and the last norm bias of mlp_2 -- it shifts
    the pooled global feature of every cloud alike, so seg_net[0]'s input moves by the same vector on every row and seg_net[1] (train-mode
    BatchNorm over all rows) takes it out again"""
    if not k.endswith(".bias") or k.startswith("seg_net.12"):
        return False
    seq = k.rsplit(".", 2)[0]
    if seq.endswith("mlp_2") and k.split(".")[-2] == "7":
        return True
    return seq in CONV_SEQS[kind] and int(k.split(".")[-2]) % 3 == 0


@pytest.mark.parametrize("path", ["kernel", "materialised"])
@pytest.mark.parametrize("kind", ["pointnet", "pointnet_basic"])
def test_model_train_mode_vs_f64(dev, monkeypatch, kind, path):
    """both implementations of seg_net[0..2] (the kernel and PAPC_SEG_CONCAT=0's materialised concat) against float64"""
    import papc_amd.segment as S
    monkeypatch.setattr(S, "_SEG_CONCAT", path == "kernel")
    B, N = 4, 1024
    m = _seeded_model(dev, kind, 31).train()
    rec = _recording(monkeypatch)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.normal(size=(B, 3, N)).astype(np.float32)).to(dev)
    gout = torch.from_numpy(rng.normal(size=(B, N, NC)).astype(np.float32)).to(dev)
    bn = m.seg_net[1]
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    logits = m(x)
    assert logits.shape == (B, N, NC)
    dec = _decisions(kind, rec)
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.named_parameters()}
    ref = _ref(kind)(P, x.double().cpu(), train=True, dec=dec)
    assert_close(_np(logits), _np(ref), BAR, "%s train logits" % kind)
    if path == "kernel":    # seg_net.1's running statistics: paddle's momentum rule on the batch statistics of the layer's pre-BN output
        yk = rec["concat"][0].grad_fn.saved_tensors[3].double()
        assert_close(_np(bn.running_mean), _np(0.9 * rm0.double() + 0.1 * yk.mean(0)), BAR, "seg_net.1 running mean")
        assert_close(_np(bn.running_var), _np(0.9 * rv0.double() + 0.1 * yk.var(0, unbiased=False)), BAR, "seg_net.1 running var")
    logits.backward(gout)
    ref.backward(gout.double().cpu())
    bad = []
    for k, p in m.named_parameters():
        g, r = p.grad, P[k].grad
        assert g is not None, k
        if _is_conv_bias_before_bn(kind, k):     # a gradient that is ~0 on both sides
            wk = k[:-4] + "weight"
            assert float((g.double().cpu() - r).abs().max()) <= 1e-4 * float(P[wk].grad.abs().max()), k
            continue
        try:
            assert_close(_np(g), _np(r), BAR, "d " + k)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad


@pytest.mark.parametrize("kind", ["pointnet", "pointnet_basic"])
def test_model_eval_mode_vs_f64(dev, kind):
    B, N = 4, 1024
    m = _seeded_model(dev, kind, 37)
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
    ref = _ref(kind)(P, x.double().cpu(), train=False)
    assert_close(_np(logits), _np(ref), BAR, "%s eval logits" % kind)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k           # eval leaves the running statistics untouched


@pytest.mark.parametrize("kind", ["pointnet", "pointnet_basic"])
def test_materialised_concat_agrees(dev, monkeypatch, kind):
    """PAPC_SEG_CONCAT=0: the concat materialised (copyops.cat_copy) and run as the first layer of a shared-MLP stack -- a second,
    independent implementation of seg_net[0..2].  One train step each: logits, every gradient and the running statistics agree."""
    import papc_amd.segment as S
    B, N = 4, 1024
    a = _seeded_model(dev, kind, 41).train()
    b = copy.deepcopy(a)
    rng = np.random.default_rng(12)
    x = torch.from_numpy(rng.normal(size=(B, 3, N)).astype(np.float32)).to(dev)
    gout = torch.from_numpy(rng.normal(size=(B, N, NC)).astype(np.float32)).to(dev)
    monkeypatch.setattr(S, "_SEG_CONCAT", True)
    la = a(x)
    la.backward(gout)
    monkeypatch.setattr(S, "_SEG_CONCAT", False)
    lb = b(x)
    lb.backward(gout)
    assert_close(_np(la), _np(lb), BAR, "%s logits kernel vs materialised" % kind)
    # Gradients: a max-norm bar of 5e-2 only.  The two implementations' outputs differ by fp32 rounding, so a ReLU decision within rounding of
    # 0 in seg_net[0..2] or any layer after it may fall differently, and one flipped row moves a layer's gradients by ~1/sqrt(B*N) of their
    # scale (measured: up to 2e-2).  Both paths are float64-checked with pinned decisions in test_model_train_mode_vs_f64.
    bad = []
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if _is_conv_bias_before_bn(kind, k):
            continue
        rel, elem = 5e-2, float("inf")
        try:
            assert_close(_np(pa.grad), _np(pb.grad), rel, "d %s kernel vs materialised" % k, elem=elem)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad
    for (k, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        if ba.dtype == torch.float32:
            assert_close(_np(ba), _np(bb), BAR, "%s kernel vs materialised" % k)


def _train_setup(dev, kind, B=8, N=1024, seed=5):
    from papc_amd.distributed import FlatAdam, FlatParams
    torch.manual_seed(seed)
    m = _make(kind, N).to(dev).train()
    flat = FlatParams(m)
    opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.normal(size=(B, 3, N)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, NC, size=(B, N))).to(dev)
    return m, flat, opt, x, y


def _step(m, opt, x, y):
    logits = m(x)
    loss = H.softmax_cross_entropy(logits.view(-1, logits.shape[-1]), y.view(-1))
    loss.backward(H.unit_gradient(x.device))
    opt.step_dev(1.0, zero_grad=True, self_tick=True)


def _state(m, flat, opt):
    st = [flat.data, flat.grad, opt.m, opt.v, opt.t_dev] + [b for b in m.buffers()]
    st += [s.rng_state for s in (m.__dict__.get(n) for n in ("_spec_input_fc", "_spec_feature_fc")) if s is not None and s.rng_state is not None]
    return st


@pytest.mark.parametrize("kind", ["pointnet", "pointnet_basic"])
def test_train_step_bit_reproducible_and_graph_replay_equal(dev, kind):
    m, flat, opt, x, y = _train_setup(dev, kind)
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


@pytest.mark.parametrize("kind", ["pointnet", "pointnet_basic"])
def test_train_step_runs_no_library_gemm(dev, kind):
    from torch.profiler import ProfilerActivity, profile
    m, flat, opt, x, y = _train_setup(dev, kind)
    _step(m, opt, x, y)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        _step(m, opt, x, y)
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    gemmish = ("cijk", "gemm", "gemv", "bmm", "matmul", "rocblas", "hipblas", "tensile", "mfma")
    mine = lambda n: "papc::" in n.split("(")[0] or n.startswith("_ZN4papc")      # (demangled or not)
    ours = [n for n in names if mine(n)]
    for k in ("cc_fwd_kernel", "cc_bwd_kernel", "cc_fold_kernel", "cc_tail_kernel", "cc_cvec_kernel"):
        assert any(k in n for n in ours), (k, sorted(names))
    foreign = [n for n in names if not mine(n) and any(s in n.lower() for s in gemmish)]
    assert not foreign, foreign


def test_errors(dev):
    for m, n in ((PointNet_Seg(NC, 1024), 1024), (PointNet_Basic_Seg(NC, 1024), 1024)):
        m = m.to(dev)
        with pytest.raises(_lib.PapcError, match="1000.*%d|%d.*1000" % (n, n)):
            m(torch.zeros(2, 3, 1000, device=dev))
        with pytest.raises(_lib.PapcError):
            m([torch.zeros(2, 3, n), None])                 # a CPU tensor
        with pytest.raises(_lib.PapcError):
            m.cpu()(torch.zeros(2, 3, n))


@pytest.mark.parametrize("kind", ["pointnet", "pointnet_basic"])
def test_seg_loader_batch_to_loss(dev, kind):
    from papc_amd.datasets import PNSegDataLoader
    N = 1024
    rng = np.random.default_rng(21)

    def opener(path):           # a small synthetic ShapeNet-part file (the loader's h5 keys)
        return {"data": rng.normal(size=(5, N, 3)).astype(np.float32), "label": rng.integers(0, 16, size=(5, 1)),
                "pid": rng.integers(0, NC, size=(5, N))}
    gen = PNSegDataLoader(max_point=N, batchsize=4, path="shapenet", mode="test", opener=opener)
    batch, target = next(iter(gen()))
    m = _seeded_model(dev, kind, 55).train()
    logits = m(batch)                                           # the source's [data, label] batch, as it comes
    assert logits.shape == (4, N, NC)
    tgt = torch.from_numpy(target.reshape(-1)).to(dev)
    loss = H.softmax_cross_entropy(logits.view(-1, NC), tgt)
    loss.backward(H.unit_gradient(dev))
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
