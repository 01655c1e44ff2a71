"""The PointPillars detection loss on the GPU (papc_amd/detloss.py on csrc/detloss.hip) against the float64 restatement tests/detloss_ref.py.

Shapes: B = 2; A in {1, 63, 64, 65, 257} and 513 -- the main pass gives a workgroup 256 anchors, so 513 is one more than a multiple of that and
spans three workgroups per sample (and the count pass's 1024 labels per workgroup are not filled) --; C in {1, 3}.

Bound: the project's activation tolerance (test_gpu_fp.py's 1e-5) as |got - ref| <= 1e-5 (|ref| + max |ref| of that tensor).  Every loss term
is non-negative, so a sum of them inherits the terms' relative error and takes the same bound.  `cared` is integer-derived: exact.
"""
import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import detloss as D
from tests import detloss_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
A_MULTI = 513                       # 2 * 256 + 1: three workgroups of the main pass per sample
SHAPES_A = (1, 63, 64, 65, 257, A_MULTI)
CW = (1.0, 0.5, 2.0, 1.0, 1.5, 1.0, 0.75)
TINY = float(np.finfo(np.float32).tiny)      # the smallest normal float

# every setting the issue names, in six combinations; `labels`: the batch's label pattern (see _labels)
CONFIGS = {
    "yaml": dict(loss_norm_type="NormByNumPositives", alpha=0.25, gamma=2.0, encode_rad_error_by_sin=False, dir=True, labels="mixed+nopos"),
    "examples-g1.5-sin-cw": dict(loss_norm_type="NormByNumExamples", alpha=0.25, gamma=1.5, encode_rad_error_by_sin=True, dir=True,
                                 code_weights=CW, labels="dontcare+allpos"),
    "posneg-sigmoid-sin-nodir": dict(loss_norm_type="NormByNumPosNeg", alpha=None, gamma=0.0, encode_rad_error_by_sin=True, dir=False,
                                     code_weights=CW, labels="mixed+nopos"),
    "posneg-focal-weights": dict(loss_norm_type="NormByNumPosNeg", alpha=0.25, gamma=2.0, encode_rad_error_by_sin=False, dir=True,
                                 code_weights=CW, pos_cls_weight=1.5, neg_cls_weight=0.5, loc_weight=1.25, cls_weight=0.75,
                                 direction_loss_weight=0.2, labels="dontcare+allpos"),
    "examples-sigmoid-nodir": dict(loss_norm_type="NormByNumExamples", alpha=None, gamma=0.0, encode_rad_error_by_sin=False, dir=False,
                                   labels="dontcare+allpos"),
    "positives-g1.5-sin-i32": dict(loss_norm_type="NormByNumPositives", alpha=0.25, gamma=1.5, encode_rad_error_by_sin=True, dir=True,
                                   sigma=2.0, labels="mixed+nopos", int32=True),
}


def _labels(pattern, A, C, g):
    """[2, A] int64.  mixed: don't care / negative / every class at random, the first anchors positive (they carry the special direction sums);
    nopos: negatives and don't-cares only (the clip of the normalisers at 1); dontcare: all -1; allpos: every anchor a class."""
    mixed = torch.randint(-1, C + 1, (A,), generator=g)
    mixed[:3] = torch.randint(1, C + 1, (min(3, A),), generator=g)
    rows = {"mixed": mixed, "nopos": torch.randint(-1, 1, (A,), generator=g), "dontcare": torch.full((A,), -1),
            "allpos": torch.randint(1, C + 1, (A,), generator=g)}
    return torch.stack([rows[p] for p in pattern.split("+")])


def _inputs(A, C, cfg, seed=0):
    """float32 CPU tensors.  Among the random values: logits at +-30 and +-90 (from A = 63 on), box diffs exactly on the smooth-L1 knee
    1 / sigma^2 (both signs), direction sums of exactly 0.0 and +- the smallest normal float (on positive anchors where the pattern has any)."""
    g = torch.Generator().manual_seed(1000 * A + 10 * C + seed)
    B = 2
    tgt = torch.randn(B, A, 7, generator=g)
    box = tgt + 0.3 * torch.randn(B, A, 7, generator=g)
    cls = 3 * torch.randn(B, A, C, generator=g)
    dirp = 2 * torch.randn(B, A, 2, generator=g)
    anchors = torch.randn(B, A, 7, generator=g)
    labels = _labels(cfg["labels"], A, C, g)
    flat = cls.view(-1)
    if flat.numel() >= 24:          # (A = 1: a reduced sum would be ONE term of 1e-40, below the range float32 holds to 1e-5 relative)
        for i, v in enumerate((30.0, -30.0, 90.0, -90.0)):
            flat[5 * i] = v
            flat[flat.numel() - 1 - 3 * i] = v
    knee = np.float32(1.0) / (np.float32(cfg.get("sigma", 3.0)) ** 2)
    cw = cfg.get("code_weights", (1.0,) * 7)
    for b in range(B):
        for j, k in enumerate((0, 3, 1)):
            a = (2 + j) % A
            tgt[b, a, k] = 0.0
            box[b, a, k] = float(knee) / cw[k] * (-1.0 if j == 1 else 1.0)
        for j, v in enumerate((0.0, TINY, -TINY)):
            a = j % A
            tgt[b, a, 6] = v
            anchors[b, a, 6] = 0.0
    return box, cls, dirp, labels, tgt, anchors


def _kw(cfg, C):
    kw = {k: v for k, v in cfg.items() if k not in ("dir", "labels", "int32")}
    kw["num_class"] = C
    return kw


def _close(got, ref, what, tol=TOL):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ref = ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), what + ": not finite"
    bound = tol * (np.abs(ref) + np.abs(ref).max())
    err = np.abs(got - ref)
    assert (err <= bound).all(), "%s: error %.3e over the bound %.3e" % (what, err.max(), bound.flat[err.argmax()])


VALUES = ("loss", "loc_loss_reduced", "cls_loss_reduced", "dir_loss_reduced", "cls_pos_loss", "cls_neg_loss", "cls_loss", "loc_loss")
_REF = {}


def _reference(A, C, name, upstream):
    """the float64 result and gradients of one case, computed once and shared"""
    key = (A, C, name, upstream)
    if key not in _REF:
        cfg = CONFIGS[name]
        box, cls, dirp, labels, tgt, anchors = _inputs(A, C, cfg)
        leaves = [t.double().requires_grad_() for t in ((box, cls, dirp) if cfg["dir"] else (box, cls))]
        r = R.pointpillars_loss(leaves[0], leaves[1], leaves[2] if cfg["dir"] else None, labels, tgt, anchors, **_kw(cfg, C))
        (r["loss"] * upstream).backward()
        _REF[key] = ({k: r[k].detach() for k in VALUES + ("cared",)}, [t.grad for t in leaves])
    return _REF[key]


def _run(dev, A, C, name, upstream, fused=None, inputs=None):
    cfg = CONFIGS[name]
    box, cls, dirp, labels, tgt, anchors = inputs if inputs is not None else _inputs(A, C, cfg)
    if cfg.get("int32"):
        labels = labels.to(torch.int32)
    leaves = [t.to(dev).requires_grad_() for t in ((box, cls, dirp) if cfg["dir"] else (box, cls))]
    r = D.pointpillars_loss(leaves[0], leaves[1], leaves[2] if cfg["dir"] else None, labels.to(dev), tgt.to(dev), anchors.to(dev),
                            fused=fused, **_kw(cfg, C))
    (r["loss"] * upstream).backward()
    return r, [t.grad for t in leaves]


def _compare(r, grads, ref, gref, tol=TOL):
    for k in VALUES:
        _close(r[k], ref[k], k, tol)
    assert torch.equal(r["cared"].cpu(), ref["cared"]) and r["cared"].dtype == torch.bool
    for what, a, b in zip(("d loss / d box_preds", "d loss / d cls_preds", "d loss / d dir_preds"), grads, gref):
        _close(a, b, what, tol)


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("A", SHAPES_A)
def test_parity_with_the_float64_reference(dev, A, C, name):
    ref, gref = _reference(A, C, name, 0.7)
    r, grads = _run(dev, A, C, name, 0.7)
    _compare(r, grads, ref, gref)
    assert r["loss"].grad_fn is not None and type(r["loss"].grad_fn).__name__.startswith("_DetLoss")      # the node, not torch ops


@pytest.fixture
def torch_flavour(monkeypatch):
    monkeypatch.setattr(D, "_DET_LOSS", False)          # what PAPC_DET_LOSS=0 sets at import


@pytest.mark.parametrize("A,C,name", [(A_MULTI, 3, "examples-g1.5-sin-cw"), (65, 1, "yaml"), (257, 3, "posneg-focal-weights"),
                                      (64, 1, "posneg-sigmoid-sin-nodir")])
def test_flavours_agree(dev, torch_flavour, A, C, name):
    """PAPC_DET_LOSS=0 (torch ops on the device) against the default, within twice the bound; the torch-op flavour itself holds the bound"""
    assert not D.fused_enabled()
    r0, g0 = _run(dev, A, C, name, 0.7)
    assert not type(r0["loss"].grad_fn).__name__.startswith("_DetLoss")
    r1, g1 = _run(dev, A, C, name, 0.7, fused=True)
    _compare(r0, g0, {k: r1[k].cpu() for k in VALUES + ("cared",)}, [g.cpu() for g in g1], 2 * TOL)
    _compare(r0, g0, *_reference(A, C, name, 0.7))


def test_two_runs_give_the_same_bits(dev):
    for C, name in ((1, "yaml"), (3, "examples-g1.5-sin-cw")):
        r1, g1 = _run(dev, A_MULTI, C, name, 0.7)
        r2, g2 = _run(dev, A_MULTI, C, name, 0.7)
        for k in VALUES:
            assert torch.equal(r1[k], r2[k]), k
        for a, b in zip(g1, g2):
            assert torch.equal(a, b)


def test_graph_replay_on_refreshed_inputs_matches_eager(dev):
    """no host synchronisation: the node captures on one stream, and a replay on new values reproduces the eager result bit for bit"""
    A, C, name = A_MULTI, 3, "examples-g1.5-sin-cw"
    cfg = CONFIGS[name]
    first, second = _inputs(A, C, cfg, seed=1), _inputs(A, C, cfg, seed=2)
    static = [t.to(dev) for t in first]
    for t in static[:3]:
        t.requires_grad_()
    up = torch.tensor(0.7, device=dev)

    def step():
        r = D.pointpillars_loss(*static, **_kw(cfg, C))
        return [r[k] for k in VALUES] + list(torch.autograd.grad(r["loss"], static[:3], grad_outputs=up))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            outs = step()
    torch.cuda.current_stream().wait_stream(s)
    with torch.no_grad():
        for t, v in zip(static, second):
            t.copy_(v.to(dev))
    g.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    eager = step()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(replayed, eager)):
        assert torch.equal(a, b), "output %d of the replay differs from the eager run" % i
    want, gwant = _run(dev, A, C, name, 0.7, inputs=second)
    assert torch.equal(replayed[0], want["loss"]) and torch.equal(replayed[len(VALUES)], gwant[0])


def test_unsupported_arguments_raise(dev):
    B, A = 2, 8
    z = lambda *s: torch.zeros(*s, device=dev)      # noqa: E731
    labels = torch.zeros(B, A, dtype=torch.int64, device=dev)
    assert D.fused_enabled()
    with pytest.raises(_lib.PapcError, match="C=9"):
        D.pointpillars_loss(z(B, A, 7), z(B, A, 9), z(B, A, 2), labels, z(B, A, 7), z(B, A, 7), num_class=9)
    with pytest.raises(_lib.PapcError, match="encode_background_as_zeros"):
        D.pointpillars_loss(z(B, A, 7), z(B, A, 2), z(B, A, 2), labels, z(B, A, 7), z(B, A, 7), num_class=1, encode_background_as_zeros=False)
    with pytest.raises(_lib.PapcError, match="code size 8"):
        D.pointpillars_loss(z(B, A, 8), z(B, A, 1), z(B, A, 2), labels, z(B, A, 8), z(B, A, 7), num_class=1, box_code_size=8)
    with pytest.raises(_lib.PapcError, match="codewise"):
        D.pointpillars_loss(z(B, A, 7), z(B, A, 1), z(B, A, 2), labels, z(B, A, 7), z(B, A, 7), num_class=1, codewise=False)


@pytest.mark.parametrize("C", [1, 3])
def test_rpn_views_equal_their_contiguous_form(dev, C):
    """[B, H, W, n k] maps that are permuted views of NCHW tensors (H = 3, W = 5, n = 2) against their contiguous [B, A, k] form: the same
    bits, and the gradients arrive in the NCHW leaves"""
    B, H, W, n = 2, 3, 5, 2
    A, cfg = H * W * n, CONFIGS["yaml"]
    box, cls, dirp, labels, tgt, anchors = [t.to(dev) for t in _inputs(A, C, cfg)]
    nchw = [t.reshape(B, H, W, n * k).permute(0, 3, 1, 2).contiguous().requires_grad_() for t, k in ((box, 7), (cls, C), (dirp, 2))]
    views = [t.permute(0, 2, 3, 1) for t in nchw]
    assert not views[0].is_contiguous()
    r = D.pointpillars_loss(*views, labels, tgt.reshape(B, H, W, n * 7), anchors.reshape(B, H, W, n, 7), **_kw(cfg, C))
    (r["loss"] * 0.7).backward()
    flat = [t.clone().requires_grad_() for t in (box, cls, dirp)]
    r2 = D.pointpillars_loss(*flat, labels, tgt, anchors, **_kw(cfg, C))
    (r2["loss"] * 0.7).backward()
    for k in VALUES:
        assert torch.equal(r[k], r2[k]), k
    assert torch.equal(r["cared"], r2["cared"]) and r["cls_preds"] is views[1]
    for a, b, k in zip(nchw, flat, (7, C, 2)):
        assert torch.equal(a.grad.permute(0, 2, 3, 1).reshape(B, A, k), b.grad)
