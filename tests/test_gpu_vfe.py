"""GPU tests of the VFE models (papc_amd.models.VFE_Clas / VFE_Seg): the K-looped concat-conv kernels (csrc/cloud_concat_k.hip) against
float64 on the materialised concat, the whole models against a float64 restatement (tests/vfe_ref.py) in train and eval mode, agreement with
the materialised path (PAPC_VFE_CONCAT=0), bit-reproducible and graph-replayable train steps, no library GEMM in a step, the reference's own
run (tests/golden/ref_model_vfe_*.npz), the error paths and a loader batch through to the loss."""
import copy

import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import head as H
from papc_amd.models import VFE_Clas, VFE_Seg
from tests import concat_cases, vfe_ref
from tests.ref_fixtures import SEG_STRIDE, gold, recorded_state
from tests.util import assert_close, copy_into_model, kernel_decisions, seeded_model_state

pytestmark = pytest.mark.gpu
BAR = 2e-4          # the project's model-level bar (as tests/test_gpu_pointnet_seg.py)
NC = {"clas": 16, "seg": 50}
KINDS = ["clas", "seg"]


def _np(t):
    return t.detach().double().cpu().numpy()


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------

# (B, N): a cloud smaller than a row tile; clouds that straddle 128-row tiles, the last segment of a cloud 72 rows; seven full segments + 104 rows
@pytest.mark.parametrize("cp,cg,cout", [(256, 256, 64), (256, 1280, 512), (64, 64, 128), (192, 2304, 64)])
@pytest.mark.parametrize("B,N", [(1, 64), (3, 200), (2, 1000)])
def test_concat_k_kernels_vs_f64(dev, B, N, cp, cg, cout):
    from papc_amd.vfe import FAMILY
    tag = "B=%d N=%d Cp=%d Cg=%d Cout=%d" % (B, N, cp, cg, cout)
    concat_cases.check_kernels_vs_f64(FAMILY, dev, B, N, cp, cg, cout, 1000 * B + N + cg + cout, BAR, tag, repeat_forward=True)


def test_both_families_on_a_shape_both_take(dev):
    """Cp = 64, Cg = 128, Cout = 512, B = 2, N = 130 (a full 128-row segment plus 2 rows per cloud, a row tile that straddles the two clouds):
    both families hold to float64, and their c is bit-equal -- one kernel (cc_cvec_kernel) serves both"""
    from papc_amd import segment, vfe
    B, N, cp, cg, cout = 2, 130, 64, 128, 512
    assert segment.kernel_ok(cp, cg, cout) and vfe.kernel_ok(cp, cg, cout)
    cvec = [concat_cases.check_kernels_vs_f64(fam, dev, B, N, cp, cg, cout, 77, BAR, "%s B=2 N=130" % fam.fwd, repeat_forward=True)
            for fam in (segment.FAMILY, vfe.FAMILY)]
    assert torch.equal(cvec[0], cvec[1])


def test_concat_k_rejects_other_shapes(dev):
    lib = _lib.load()
    t = torch.zeros(4 * 8, 2368 + 320, device=dev)
    p = t.data_ptr()
    for cp, cg, cout, what in ((320, 256, 64, "Cp=320"), (32, 256, 64, "Cp=32"), (256, 256, 576, "Cout=576"), (256, 96, 64, "Cg=96"),
                               (256, 2368, 64, "Cg=2368")):
        with pytest.raises(_lib.PapcError, match=what):
            _lib.check(lib.papc_cloud_concat_k_f32(p, 320, p, p, None, 4, 8, cp, cg, cout, p, p, None, _lib.stream_ptr()), "fwd")
        with pytest.raises(_lib.PapcError, match=what):
            _lib.check(lib.papc_cloud_concat_k_bwd_f32(p, p, p, p, p, p, p, p, p, 320, p, p, 4, 8, cp, cg, cout, p, 320, 0, p, p, p, None, p, 1 << 20,
                                                       _lib.stream_ptr()), "bwd")
    with pytest.raises(_lib.PapcError, match="null"):
        _lib.check(lib.papc_cloud_concat_k_f32(None, 256, p, p, None, 4, 8, 256, 256, 64, p, p, None, _lib.stream_ptr()), "fwd")
    with pytest.raises(_lib.PapcError, match="workspace"):
        _lib.check(lib.papc_cloud_concat_k_bwd_f32(p, p, p, p, p, p, p, p, p, 256, p, p, 4, 8, 256, 256, 64, p, 256, 0, p, p, p, None, p, 16,
                                                   _lib.stream_ptr()), "bwd")


# ---- the models -------------------------------------------------------------------------------------------------------------------------

def _make(kind, N):
    return VFE_Clas(NC[kind], N) if kind == "clas" else VFE_Seg(256, NC[kind], N)


def _ref(kind):
    return vfe_ref.vfe_clas if kind == "clas" else vfe_ref.vfe_seg


def _seeded_model(dev, kind, seed, N=256):
    m = _make(kind, N).to(dev)
    st = seeded_model_state(m, seed)
    rng = np.random.default_rng(seed + 1)
    for name, mod in m.named_modules():         # (the norms of seg_net: seeded_model_state knows norms by "bn" / "norm" in their names)
        if isinstance(mod, torch.nn.BatchNorm1d):
            c = mod.num_features
            st[name + ".weight"] = (rng.uniform(0.5, 1.5, size=c) * rng.choice([1.0, 1.0, 1.0, -1.0], size=c)).astype(np.float32)
            st[name + ".bias"] = (rng.normal(size=c) * 0.2).astype(np.float32)
    copy_into_model(m, st)
    return m


def _recording(monkeypatch):
    """record the stack, head and concat-layer calls of a forward (their autograd nodes hold the kernels' decisions)"""
    import papc_amd.models as M
    import papc_amd.vfe as V
    rec = {"stacks": [], "head": [], "concat": [], "concat_args": []}

    def wrap(fn, key):
        def inner(*a, **k):
            out = fn(*a, **k)
            rec[key].append(out)
            if key == "concat":
                rec["concat_args"].append(a)
            return out
        return inner
    monkeypatch.setattr(M, "shared_mlp_max", wrap(M.shared_mlp_max, "stacks"))
    monkeypatch.setattr(H, "plain_head", wrap(H.plain_head, "head"))
    monkeypatch.setattr(V, "concat_k_bn_relu", wrap(V.concat_k_bn_relu, "concat"))
    return rec


def _decisions(kind, m, rec):
    names = ["pointnet_1", "pointnet_2"] + (["seg1"] if kind == "seg" else [])
    assert len(rec["stacks"]) == len(names) and len(rec["concat"]) == (2 if kind == "seg" else 1)
    dec = {}
    for nm, out in zip(names, rec["stacks"]):
        argmax, alive, masks = kernel_decisions(out)
        dec[nm] = (argmax.cpu() if argmax is not None else None, alive.cpu(), [None if mk is None else mk.cpu() for mk in masks])
    g1 = rec["concat_args"][0][1]                                      # pillars._GroupMax's output: its node saved the winners
    dec["g1"] = g1.grad_fn.saved_tensors[0].cpu()
    for nm, out in zip(["concat0", "seg0"], rec["concat"]):
        dec[nm] = (None, (out.detach() > 0).cpu(), None)
    if kind == "clas":
        assert len(rec["head"]) == 1
        saved = rec["head"][0].grad_fn.saved_tensors                   # _HeadPlain: (x0, w1, w2, w3, relu1 out, dropout(relu2) out)
        keep = m._head_spec.masks[0].bool().cpu() if m.training else None
        dec["fc"] = ((saved[4] > 0).cpu(), (saved[5] > 0).cpu(), keep)   # (a dropped entry is zero on both sides whatever its ReLU decision)
    return dec


def _exactly_zero_gradient(kind, k):
    """parameters whose exact gradient is ~0 (held as test_gpu_pointnet_seg._is_conv_bias_before_bn does): every conv bias in front of a train-mode
    norm; in VFE_Seg also the bias of vfe.pointnet_2.mlp_2.2._batch_norm -- it shifts x2 of every cloud alike, so seg_net[0]'s input moves by
    the same vector on every row and seg_net[1] (train-mode BatchNorm over all rows) takes it out again.  -> the sibling weight's name, or None"""
    if k.endswith("._conv.bias"):
        return k[:-4] + "weight"
    if k.startswith("seg_net.") and k.endswith(".bias") and not k.startswith("seg_net.12") and int(k.split(".")[1]) % 3 == 0:
        return k[:-4] + "weight"
    if kind == "seg" and k == "vfe.pointnet_2.mlp_2.2._batch_norm.bias":
        return k[:-4] + "weight"
    return None


def _concat_layers(kind, m):
    b = m.vfe.pointnet_2.mlp_1[0]
    return [(b._conv, b._batch_norm)] + ([(m.seg_net[0], m.seg_net[1])] if kind == "seg" else [])


def _inputs(dev, kind, B, N, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.normal(size=(B, 3, N)).astype(np.float32)).to(dev)
    shape = (B, NC[kind]) if kind == "clas" else (B, N, NC[kind])
    gout = torch.from_numpy(rng.normal(size=shape).astype(np.float32)).to(dev)
    return x, gout


@pytest.mark.parametrize("path", ["kernel", "materialised"])
@pytest.mark.parametrize("kind", KINDS)
def test_model_train_mode_vs_f64(dev, monkeypatch, kind, path):
    """both implementations of the concat layers (the kernels and PAPC_VFE_CONCAT=0's materialised concat) against float64; seg: Cg = 512"""
    import papc_amd.vfe as V
    monkeypatch.setattr(V, "_VFE_CONCAT", path == "kernel")
    B, N = 4, 256
    m = _seeded_model(dev, kind, 31).train()
    if kind == "clas":
        m.__dict__["_head_spec"] = H.HeadSpec()
        m._head_spec.export_masks = True
    rec = _recording(monkeypatch)
    x, gout = _inputs(dev, kind, B, N, 3)
    run0 = [(bn.running_mean.clone(), bn.running_var.clone()) for _, bn in _concat_layers(kind, m)]
    logits = m(x)
    assert logits.shape == gout.shape
    dec = _decisions(kind, m, rec)
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.named_parameters()}
    ref = _ref(kind)(P, x.double().cpu(), train=True, dec=dec)
    assert_close(_np(logits), _np(ref), BAR, "VFE %s train logits" % kind)
    # the concat layers' running statistics: paddle's momentum rule on the batch statistics of the layer's pre-BN output, in float64 from the
    # layer's own inputs
    for (conv, bn), (rm0, rv0), a in zip(_concat_layers(kind, m), run0, rec["concat_args"]):
        cat = torch.cat([a[0].detach().double(), a[1].detach().double().repeat_interleave(N, 0)], 1)
        y = cat @ conv.weight.detach().double().squeeze(-1).t() + conv.bias.detach().double()
        assert_close(_np(bn.running_mean), _np(0.9 * rm0.double() + 0.1 * y.mean(0)), BAR, "concat layer running mean")
        assert_close(_np(bn.running_var), _np(0.9 * rv0.double() + 0.1 * y.var(0, unbiased=False)), BAR, "concat layer running var")
    logits.backward(gout)
    ref.backward(gout.double().cpu())
    bad = []
    for k, p in m.named_parameters():
        g, r = p.grad, P[k].grad
        assert g is not None, k
        wk = _exactly_zero_gradient(kind, k)
        if wk is not None:     # a gradient that is ~0 on both sides
            assert float((g.double().cpu() - r).abs().max()) <= 1e-4 * float(P[wk].grad.abs().max()), k
            continue
        try:
            assert_close(_np(g), _np(r), BAR, "d " + k)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad


@pytest.mark.parametrize("kind", KINDS)
def test_model_eval_mode_vs_f64(dev, monkeypatch, kind):
    """model.eval(): the running statistics normalise and stay untouched; a backward through the frozen norms gives the restatement's gradients"""
    B, N = 4, 256
    m = _seeded_model(dev, kind, 37)
    rng = np.random.default_rng(9)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(torch.from_numpy(rng.normal(size=mod.num_features).astype(np.float32) * 0.1))
                mod.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 2.0, size=mod.num_features).astype(np.float32)))
    m.eval()
    x, gout = _inputs(dev, kind, B, N, 10)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        logits = m(x)
    S = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    ref = _ref(kind)(S, x.double().cpu(), train=False)
    assert_close(_np(logits), _np(ref), BAR, "VFE %s eval logits" % kind)
    # the eval-mode backward, decisions pinned
    rec = _recording(monkeypatch)
    logits = m(x)
    dec = _decisions(kind, m, rec)
    P = dict(S)
    for k, _ in m.named_parameters():
        P[k] = S[k].clone().requires_grad_(True)
    ref = _ref(kind)(P, x.double().cpu(), train=False, dec=dec)
    assert_close(_np(logits), _np(ref), BAR, "VFE %s eval logits, decisions pinned" % kind)
    logits.backward(gout)
    ref.backward(gout.double().cpu())
    bad = []
    for k, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        try:
            assert_close(_np(p.grad), _np(P[k].grad), BAR, "eval d " + k)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k           # eval leaves the running statistics untouched


@pytest.mark.parametrize("kind", KINDS)
def test_materialised_concat_agrees(dev, monkeypatch, kind):
    """PAPC_VFE_CONCAT=0: the concats materialised (copyops.cat_copy) and run as one-layer shared-MLP stacks -- a second, independent
    implementation.  One train step each: logits, every gradient and the running statistics agree."""
    import papc_amd.vfe as V
    B, N = 4, 256
    a = _seeded_model(dev, kind, 41).train()
    for mod in a.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0                                # (the two models would draw different masks)
    b = copy.deepcopy(a)
    x, gout = _inputs(dev, kind, B, N, 12)
    monkeypatch.setattr(V, "_VFE_CONCAT", True)
    la = a(x)
    la.backward(gout)
    monkeypatch.setattr(V, "_VFE_CONCAT", False)
    lb = b(x)
    lb.backward(gout)
    assert_close(_np(la), _np(lb), BAR, "VFE %s logits kernel vs materialised" % kind)
    # Gradients: a max-norm bar of 5e-2 only, for the reason given in test_gpu_pointnet_seg.test_materialised_concat_agrees: the two
    # implementations' outputs differ by fp32 rounding, so a ReLU or max decision within rounding of a tie may fall differently, and one flipped
    # row moves a layer's gradients by ~1/sqrt(B*N) of their scale.  Both paths are float64-checked with pinned decisions above.
    bad = []
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if _exactly_zero_gradient(kind, k) is not None:
            continue
        try:
            assert_close(_np(pa.grad), _np(pb.grad), 5e-2, "d %s kernel vs materialised" % k, elem=float("inf"))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad
    for (k, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        if ba.dtype == torch.float32:
            assert_close(_np(ba), _np(bb), BAR, "%s kernel vs materialised" % k)


def _train_setup(dev, kind, B=8, N=256, seed=5):
    from papc_amd.distributed import FlatAdam, FlatParams
    torch.manual_seed(seed)
    m = _make(kind, N).to(dev).train()
    flat = FlatParams(m)
    opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.normal(size=(B, 3, N)).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, NC[kind], size=(B,) if kind == "clas" else (B, N))).to(dev)
    return m, flat, opt, x, y


def _step(m, opt, x, y):
    logits = m(x)
    loss = H.softmax_cross_entropy(logits.view(-1, logits.shape[-1]), y.view(-1))
    loss.backward(H.unit_gradient(x.device))
    opt.step_dev(1.0, zero_grad=True, self_tick=True)


def _state(m, flat, opt):
    st = [flat.data, flat.grad, opt.m, opt.v, opt.t_dev] + [b for b in m.buffers()]
    spec = m.__dict__.get("_head_spec")
    if spec is not None and spec.rng_state is not None:
        st.append(spec.rng_state)
    return st


@pytest.mark.parametrize("kind", KINDS)
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


@pytest.mark.parametrize("kind", KINDS)
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
    mine = lambda n: "papc::" in n.split("(")[0] or n.startswith("_ZN4papc")      # noqa: E731  (demangled or not)
    ours = [n for n in names if mine(n)]
    for k in ("cck_fwd_kernel", "cc_cvec_kernel", "cck_wt_kernel", "cck_colsum_kernel", "cck_fold_kernel", "cc_tail_kernel"):
        assert any(k in n for n in ours), (k, sorted(names))
    foreign = [n for n in names if not mine(n) and any(s in n.lower() for s in gemmish)]
    assert not foreign, foreign


# ---- the reference's own run ----------------------------------------------------------------------------------------------------------------

def _pinned(kind, dev):
    from papc_amd import checkpoint
    z = gold("ref_model_vfe_" + kind)
    m = VFE_Clas() if kind == "clas" else VFE_Seg()
    state, _ = recorded_state(z)
    checkpoint.import_state(m, state, strict=True)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0                                # the recorder's forwards draw no dropout mask
    return m.to(dev), z


def _elem(z, key):
    """test_gpu_reference_pin._elem's rule: 100 x the max-norm bar, never tighter than 3 x the reference's own float32-mode deviation"""
    return max(100.0 * BAR, 3.0 * float(z["own32_" + key][1]))


@pytest.mark.parametrize("kind", KINDS)
def test_model_against_the_reference_run(dev, kind, monkeypatch):
    from papc_amd import models as M
    lay = gold("ref_layers")
    m, z = _pinned(kind, dev)
    x = torch.from_numpy(np.ascontiguousarray(np.transpose(lay["cloud"], (0, 2, 1)))).to(dev)          # B = 2, N = 1024
    B, _, N = x.shape
    args = (x,) if kind == "clas" else ([x, torch.from_numpy(lay["seg_labels"]).to(dev)],)
    sl = (lambda a: a[:, ::SEG_STRIDE]) if kind == "seg" else (lambda a: a)
    m.train()
    with torch.no_grad():
        tl = m(*args)
    assert_close(sl(_np(tl)), z["train_logits"], rel=BAR, what="vfe_%s train logits" % kind, elem=_elem(z, "eval_logits"))
    mods = dict(m.named_modules())
    for tag in ("first", "last"):
        bn = mods[str(z[tag + "_norm"][0])]
        assert_close(_np(bn.running_mean), z[tag + "_mean"], rel=BAR, what="vfe_%s %s running mean" % (kind, z[tag + "_norm"][0]))
        assert_close(_np(bn.running_var), z[tag + "_var"], rel=BAR, what="vfe_%s %s running variance" % (kind, z[tag + "_norm"][0]))
    m.eval()
    with torch.no_grad():
        ev = m(*args)
    assert_close(sl(_np(ev)), z["eval_logits"], rel=BAR, what="vfe_%s eval logits" % kind, elem=_elem(z, "eval_logits"))
    # the tensor entering the head, from a second seeded copy in train mode
    twin, _ = _pinned(kind, dev)
    twin.train()
    with torch.no_grad():
        x1, g1, x2 = twin.vfe.features(x, True)
    if kind == "clas":
        h = _np(x2)                                                                                    # fc's input [B, max_points]
    else:                                                                                              # seg_net's input [B, 1536, N], every 32nd point
        rows = torch.cat([x1.view(B, N, -1), g1.view(B, 1, -1).expand(B, N, -1), x2.view(B, 1, -1).expand(B, N, -1)], 2)
        h = _np(rows.transpose(1, 2))[..., ::SEG_STRIDE]
    assert_close(h.reshape(z["head_in"].shape), z["head_in"], rel=BAR, what="vfe_%s head input" % kind, elem=_elem(z, "head_in"))


# ---- errors, the loader ---------------------------------------------------------------------------------------------------------------------

def test_errors(dev):
    for kind in KINDS:
        m = _make(kind, 256).to(dev)
        with pytest.raises(_lib.PapcError, match="200.*256|256.*200"):
            m(torch.zeros(2, 3, 200, device=dev))
        with pytest.raises(_lib.PapcError):
            m(torch.zeros(2, 3, 256))                       # a CPU tensor
        with pytest.raises(_lib.PapcError):
            m.cpu()(torch.zeros(2, 3, 256))


@pytest.mark.parametrize("kind", KINDS)
def test_loader_batch_to_loss(dev, kind):
    from papc_amd.datasets import DataLoader
    N = 256
    rng = np.random.default_rng(21)

    def opener(path):           # a small synthetic file (the loader's h5 keys)
        return {"data": rng.normal(size=(5, N, 3)).astype(np.float32), "label": rng.integers(0, 16, size=(5, 1)),
                "pid": rng.integers(0, NC["seg"], size=(5, N))}
    gen = DataLoader("vfe", N, 4, path="data", mode1=kind, mode2="test", opener=opener)
    batch, target = next(iter(gen()))
    m = _seeded_model(dev, kind, 55).train()
    logits = m(batch)                                           # the source's batch, as it comes
    assert logits.shape == ((4, NC[kind]) if kind == "clas" else (4, N, NC[kind]))
    tgt = torch.from_numpy(target.reshape(-1)).to(dev)
    loss = H.softmax_cross_entropy(logits.view(-1, NC[kind]), tgt)
    loss.backward(H.unit_gradient(dev))
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
