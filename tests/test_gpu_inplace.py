"""The in-place gradient path (distributed.FlatParams: every parameter carries ``_papc_inplace_grad``, the autograd nodes take the accumulate
flavour of their backward kernels, add into ``.grad`` and hand autograd ``None``; stack.SharedMLPStack defers its folds to folds.pending())
held to the autograd path in every model.

The reference is the AUTOGRAD TWIN: a ``copy.deepcopy`` of the model that is not wrapped in FlatParams.  Both copies run the same kernels on
bit-identical forwards, so every ReLU / max / pool decision agrees, and the twin's gradients are the ones the per-model tests hold to float64
(test_model_vs_f64 and friends run on the autograd path).  Equality with the twin is sharper than any float64 bar.  ``torch.equal`` is the
"bit for bit" of this file: it differs from a comparison of the bits only in 0.0 == -0.0, which ``0 + s`` and ``s`` may differ in.

Every test asserts first that the two forwards are bit-equal (dropout p = 0: the modules allow it, as test_gpu_folds._step does) and that the
in-place path was really taken: a ``register_hook`` on every opted-in parameter of the flat copy must never see a gradient tensor -- the nodes
return ``None`` there (the engine then runs the hook with None), on the autograd path the hook receives the gradient -- except for the
parameters listed in VIA_AUTOGRAD, which reach their node through a derived tensor and come back through autograd by design
(nodeparts.grad_targets_of: "entries that are not opted-in leaf Parameters").

Tolerances.  Bit equality everywhere except:
  * FOLD_BAR = 2e-5 (max-norm, tests/test_gpu_folds.py's bar) for the tensors whose deferred fold sums in another FIXED order than the stack's
    own fold -- and only with folds.ENABLED: see _fold_order_params -- and for linear_rows' weight, whose two paths fold differently: LINEAR_ROWS;
  * ATOMIC_BAR = 1e-5 (max-norm) for the gradients behind a float-atomic sum, where the twin itself is not reproducible: NOISY;
  * a conv bias under a train-mode norm whose in-place gradient is the exact 0 (the kernels write nothing there: nodeparts.LayerSlots,
    "gradient exactly 0 -- nothing to add in place") while the twin holds autograd's rounding noise: the twin at most 1e-4 of the weight
    gradient's max, the rule of tests/test_gpu_step.py:63.
"""
import copy

import numpy as np
import pytest
import torch

from papc_amd import _lib, folds, kdnet, stack, voxnet
from papc_amd.distributed import FlatParams
from papc_amd.head import softmax_cross_entropy
from papc_amd.layers import PointNetSetAbstraction
from papc_amd.models import (KDNet, KDUNet, PointNet2_MSG_Clas, PointNet2_MSG_Seg, PointNet2_SSG_Clas, PointNet2_SSG_Seg, PointNet_Basic_Clas,
                             PointNet_Clas, PointNet_Seg, VoxNet)
from papc_amd.pillars import PillarFeatureNet
from papc_amd.synthetic import make_clouds, make_labels, make_pillars, make_start_idx
from tests.util import copy_into_model, seeded_model_state

pytestmark = pytest.mark.gpu

FOLD_BAR = 2e-5          # tests/test_gpu_folds.py::test_deferred_folds_equal_per_stack_folds: deferred vs per-stack folds, another fixed order
N = 1024


# ---- the models: (constructor, batch(dev, seed) -> args, loss(model, args)) -----------------------------------------------------------
# Shapes: each model's own _train_setup (tests/test_gpu_*.py) with the batch cut to <= 4; class / part counts of 10 and 50, so that the last
# bias (10 or 50 floats) is no multiple of 4 and FlatParams leaves a padding gap behind it.

def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _starts(B, seed, dev):
    return (_t(make_start_idx(B, N, seed), dev), _t(make_start_idx(B, 512, seed + 1), dev))


def _clas_batch(B, nc):
    def batch(dev, seed):
        return _t(make_clouds(B, N, seed), dev), _starts(B, seed, dev), _t(make_labels(B, nc, seed), dev).reshape(-1)
    return batch


def _clas_loss(m, a):
    out = m(a[0], a[1])
    return softmax_cross_entropy(out, a[2]), out


def _seg_batch(B, parts):
    def batch(dev, seed):
        cls = (np.arange(B).reshape(B, 1) * 5 + seed) % 16
        y = _t(np.random.default_rng(seed).integers(0, parts, size=B * N), dev)
        return _t(make_clouds(B, N, seed), dev), cls.astype(np.int64), _starts(B, seed, dev), y
    return batch


def _seg_loss(m, a):
    logits = m((a[0], a[1]), a[2])
    return softmax_cross_entropy(logits.reshape(-1, logits.shape[-1]), a[3]), logits


def _points_batch(B, nc, per_point):
    def batch(dev, seed):
        rng = np.random.default_rng(seed)
        x = rng.normal(size=(B, 3, N)).astype(np.float32)
        return _t(x, dev), _t(rng.integers(0, nc, size=B * N if per_point else B), dev)
    return batch


def _points_loss(m, a):
    logits = m(a[0])
    return softmax_cross_entropy(logits.reshape(-1, logits.shape[-1]), a[1]), logits


def _kd_batch(B, nc, per_point):
    def batch(dev, seed):
        rng = np.random.default_rng(seed)
        x = rng.normal(size=(B, 3, N)).astype(np.float32)
        sels = [rng.integers(0, 3, size=(B, d)) for d in kdnet.DIMS]
        return _t(x, dev), kdnet.pack_split_dims(sels, B, dev), _t(rng.integers(0, nc, size=B * N if per_point else B), dev)
    return batch


def _kd_loss(m, a):
    logits = m([a[0], a[1]])
    return softmax_cross_entropy(logits.reshape(-1, logits.shape[-1]), a[2]), logits


def _vox_batch(B, nc):
    def batch(dev, seed):
        rng = np.random.default_rng(seed)
        pts = rng.uniform(-1.0, 1.0, size=(B, 1024, 3)).astype(np.float32)
        return voxnet.occupancy_grid(_t(pts, dev)), _t(rng.integers(0, nc, size=B), dev)
    return batch


def _pfn_batch(P, T):
    def batch(dev, seed):
        voxels, nump, coors = make_pillars(P=P, T=T, seed=seed)
        gout = np.random.default_rng(seed).normal(size=(P, 64)).astype(np.float32)
        return _t(voxels, dev), _t(nump, dev), _t(coors, dev), _t(gout, dev)
    return batch


def _pfn_loss(m, a):
    out = m(a[0], a[1], a[2])
    return (out * a[3]).sum(), out


def _sa_batch(B):
    def batch(dev, seed):
        gout = np.random.default_rng(seed).normal(size=(B, 128, 512)).astype(np.float32)
        return _t(make_clouds(B, N, seed), dev), _t(make_start_idx(B, N, seed), dev), _t(gout, dev)
    return batch


def _sa_loss(m, a):
    out = m(a[0], None, a[1])[1]
    return (out * a[2]).sum(), out


CASES = {
    "ssg_clas": (lambda: PointNet2_SSG_Clas(num_classes=10), _clas_batch(4, 10), _clas_loss),
    # 16 classes: the fused head (head.usable wants fc3.out_features % 4 == 0; with 10 classes the head runs as torch modules) -- no gap then
    "ssg_clas16": (lambda: PointNet2_SSG_Clas(num_classes=16), _clas_batch(4, 16), _clas_loss),
    "msg_clas": (lambda: PointNet2_MSG_Clas(num_classes=10), _clas_batch(4, 10), _clas_loss),
    "ssg_seg": (lambda: PointNet2_SSG_Seg(num_parts=50, fp_neighbours="nearest"), _seg_batch(2, 50), _seg_loss),
    "msg_seg": (lambda: PointNet2_MSG_Seg(num_parts=50, fp_neighbours="nearest"), _seg_batch(2, 50), _seg_loss),
    "pointnet_basic_clas": (lambda: PointNet_Basic_Clas(10, N), _points_batch(4, 10, False), _points_loss),
    "pointnet_clas": (lambda: PointNet_Clas(10, N), _points_batch(4, 10, False), _points_loss),
    "pointnet_seg": (lambda: PointNet_Seg(50, N), _points_batch(4, 50, True), _points_loss),
    "kdnet": (lambda: KDNet(num_classes=10), _kd_batch(4, 10, False), _kd_loss),
    "kdunet": (lambda: KDUNet(num_classes=50), _kd_batch(4, 50, True), _kd_loss),
    "voxnet": (lambda: VoxNet(num_classes=10), _vox_batch(3, 10), _points_loss),
    # the PillarFeatureNet layer as tests/test_gpu_pfn.py::test_pfn_inplace_gradients_match_autograd sets it up
    "pfn": (lambda: PillarFeatureNet(num_filters=(64,), voxel_size=(0.16, 0.16, 4), pc_range=(0, -39.68, -3, 69.12, 39.68, 1)), _pfn_batch(300, 50),
            _pfn_loss),
    # pattern (d) only: ONE set-abstraction layer (SA1 of the SSG classifier), so that all fold jobs of a backward share one launch
    "sa_layer": (lambda: PointNetSetAbstraction(512, 0.2, 32, 3, [64, 64, 128], False), _sa_batch(4), _sa_loss),
}
MODELS = [k for k in CASES if k != "sa_layer"]
NO_GAP = ("pfn", "ssg_clas16")      # the PFN layer (64 x 9, 64, 64) has no count to choose; 16 classes: see CASES
# the models whose stacks defer folds get a second run with folds.ENABLED = False: every tensor bit-equal then (but LINEAR_ROWS and NOISY)
STACK_MODELS = ["ssg_clas16", "msg_clas", "ssg_seg", "msg_seg", "pointnet_basic_clas", "pointnet_clas", "pointnet_seg", "kdunet"]


def _wb(prefix, idx):
    return {"%s.%d.%s" % (prefix, i, s) for i in idx for s in ("weight", "bias")}


_CLAS_HEAD = {"%s.%s" % (m, s) for m in ("fc1", "bn1", "fc2", "bn2", "fc3") for s in ("weight", "bias")}
# Parameters of the flat copy whose hook DOES receive a gradient, by design: their node has no in-place flavour for them.
VIA_AUTOGRAD = {
    # 10 classes: head.usable / head.plain_usable want fc3.out_features % 4 == 0, else the head runs as torch modules (models._ClasHead._head,
    # PointNet_Basic_Clas.forward)
    "ssg_clas": _CLAS_HEAD,
    "msg_clas": _CLAS_HEAD,
    "pointnet_basic_clas": _wb("fc", (0, 2, 5)),
    # transform.tnet_fc: the 3 x 3 T-Net's last layer has 9 outputs and runs padded, "the padded node hands autograd every gradient"
    "pointnet_clas": _wb("fc", (0, 2, 5)) | _wb("input_fc", (0, 2, 4)),
    # ... and cloudconcat._CloudConcatBnRelu (seg_net[0..1]) has no accumulate flavour: it always returns dw, db, dgamma, dbeta
    "pointnet_seg": _wb("input_fc", (0, 2, 4)) | _wb("seg_net", (0, 1)),
    # layers._pad_features: D = 3 feature channels are padded to 4, the first conv weight is a zero-padded view (no leaf Parameter)
    "ssg_seg": {"sa1.mlp_convs.0.weight"},
    "msg_seg": {"sa1.conv_blocks.%d.0.weight" % i for i in range(3)},
    # models.KDUNet.forward: the transposed convs run as linear_rows on the PERMUTED weight and the REPEATED bias (no leaf Parameters)
    "kdunet": {"upsample.deconv%d.%s" % (i, s) for i in range(1, 6) for s in ("weight", "bias")},
}

# linear.linear_rows folds its dW partials with DwPartials.fold_cols in place (papc_reduce_partials_strided_f32: the slice tree) and with
# DwPartials.fold on the autograd path (papc_reduce_partials2_f32: the lane fold) -- linear.py, `if acc: part.fold_cols(...) else: part.fold(...)`:
# two fixed orders of the same partials, FOLD_BAR whatever folds.ENABLED says (one chunk of rows: the same bits)
LINEAR_ROWS = {"ssg_seg": {"conv2.weight"}, "msg_seg": {"conv2.weight"}, "pointnet_seg": {"seg_net.12.weight"}, "kdnet": {"fc.weight"},
               "kdunet": {"upsample.doubleconv5.1.weight"}, "voxnet": {"head.0.weight", "head.3.weight"}}

# Gradients behind a FLOAT-ATOMIC sum: the same terms in a run-dependent order, so that two runs of the twin itself differ in the last bits
# (measured here: up to 2e-6 of max|grad| between two runs of either copy) and bit equality with the twin is not defined.
#   * the part segmenters: the interpolation backward of fp2 / fp1 scatters with float atomics -- everything it feeds (fp3, fp2 and the three
#     SA levels; fp1, conv1 / bn1 and conv2 are ahead of it and bit-equal), tests/test_gpu_seg.py:197;
#   * PointNet2_MSG_Clas: SA2's gather-add backward runs without point lists (float-atomic row sums G) -- the first-layer dW of its branches
#     (dW_f = G^T feats) and, through dfeats, all of SA1; tests/test_gpu_models.py:338, tests/test_gpu_compact.py:427.
# Those tests' bar for that noise is 1e-5 of max|grad| (tests/test_gpu_cabi.py:214, tests/test_gpu_seg.py:198); a (near-)zero gradient -- a
# bias under a train-mode norm -- is read on the scale of its weight's gradient, whose terms it sums.
ATOMIC_BAR = 1e-5
_ENCODER = ("sa1.", "sa2.", "sa3.", "fp3.", "fp2.")
NOISY = {"ssg_seg": _ENCODER, "msg_seg": _ENCODER, "msg_clas": ("sa1.",) + tuple("sa2.conv_blocks.%d.0.weight" % i for i in range(3))}


class Pair:
    """a model wrapped in FlatParams and its autograd twin"""

    def __init__(self, case, dev, freeze=None, seed=5):
        build, self.batch, self.loss = CASES[case]
        self.case, self.dev = case, dev
        torch.manual_seed(seed)
        m = build().to(dev).train()
        copy_into_model(m, seeded_model_state(m, seed))          # non-trivial norm weights, negative ones included; no zero-initialised T-Net weight
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        self.frozen = set(freeze(m)) if freeze is not None else set()
        for n, p in m.named_parameters():
            if n in self.frozen:
                p.requires_grad_(False)
        self.twin = copy.deepcopy(m)
        self.model = m
        self.flat = FlatParams(m)
        self.fired = []
        self.names = [n for n, p in m.named_parameters() if p.requires_grad]
        for n, p in m.named_parameters():
            if getattr(p, "_papc_inplace_grad", False):
                # (the engine still runs a leaf's hooks when its node returned None, with None: only a hook that sees a TENSOR has fired)
                p.register_hook(lambda g, n=n: self.fired.append(n) if g is not None else None)
        assert sorted(n for n, p in m.named_parameters() if getattr(p, "_papc_inplace_grad", False)) == sorted(self.names)
        self.loose = set()
        self.linear_rows = LINEAR_ROWS.get(case, set())
        self.noisy = {n for n in self.names if n.startswith(NOISY.get(case, ("\0",)))}

    def step(self, args, both=True):
        """forward + backward of the flat copy (and of the twin): the forwards must be bit-equal"""
        lf, of = self.loss(self.model, args)
        if both:
            lt, ot = self.loss(self.twin, args)
            # (the outputs, not the loss: softmax_cross_entropy sums its row blocks with a float atomic, head.hip -- run-dependent last bits
            # in the VALUE of a loss over more rows than one block; its gradient does not read that sum)
            assert torch.equal(of.detach(), ot.detach()), "the two forwards differ by %.3e" % float((of - ot).abs().max())
            lt.backward()
        lf.backward()
        torch.cuda.synchronize()
        if folds.ENABLED:
            self.loose |= _fold_order_params(self.model)

    def zero(self):
        self.flat.zero_grad()
        self.twin.zero_grad(set_to_none=True)
        torch.cuda.synchronize()

    def grads(self):
        return {n: p.grad.detach().clone() for n, p in self.model.named_parameters() if p.requires_grad}

    def twin_grads(self):
        return {n: p.grad.detach().clone() for n, p in self.twin.named_parameters() if p.requires_grad}

    def gap_mask(self):
        """True at the padding elements FlatParams leaves behind a parameter whose numel is no multiple of 4"""
        gap = torch.ones(self.flat.numel, dtype=torch.bool, device=self.dev)
        for p, off in zip(self.flat.params, self.flat._offsets):
            gap[off: off + p.numel()] = False
        return gap

    def check_hooks(self):
        want = VIA_AUTOGRAD.get(self.case, set())
        fired = set(self.fired)
        assert fired == want, "hooks fired for %s, expected %s: the in-place path was not taken (or a derived-tensor parameter no longer goes through autograd)" % (
            sorted(fired - want), sorted(want - fired))


def _fold_order_params(model):
    """The conv weights whose DEFERRED fold sums in another fixed order than the stack's own fold (csrc/sa_mlp.hip), read from the plans the
    library chose (stack.LAST_PLANS):
      * the gather-add first layer (plan.lin0): its two STRIDED jobs -- the xyz and the feature column block of dW, sa_mlp.hip `defer_fold(...,
        dw + xcol0, cin, acc)` / `dw + fcol0` -- run as the lane fold in papc_fold_jobs_f32, as papc_reduce_partials_strided_f32's slice tree
        when the stack folds on its own;
      * the planes path (plan.planes): the SPLIT-K job of every layer's dW -- the in-order fold of papc_fold_jobs_f32's wide kind (or a lane
        fold, by size) against papc_pg_fold_f32.
    The dW / db jobs of every other layer keep their order (fold_lanes<16, 8> in both) and are bit-identical.
    A plan is keyed by its stack's output widths: the stack's layers are the run of consecutive conv layers of the model with these widths."""
    convs = [(n, m) for n, m in model.named_modules() if isinstance(m, (torch.nn.Conv1d, torch.nn.Conv2d))]
    out = set()
    for (_, couts), plan in stack.LAST_PLANS.items():
        L = len(couts)
        for i in range(len(convs) - L + 1):
            run = convs[i: i + L]
            if tuple(m.out_channels for _, m in run) != tuple(couts) or any(run[l + 1][1].in_channels != couts[l] for l in range(L - 1)):
                continue
            if plan["lin0"]:
                out.add(run[0][0] + ".weight")
            if plan["planes"]:
                out |= {n + ".weight" for n, _ in run}
    return out


def _compare(pair, got, ref, what, bad, same_path=False, noise_of=None):
    """Every gradient of ``got`` (the flat copy) against ``ref``: bit equality, with the documented exceptions.  ``same_path``: ``ref`` was
    made from the flat copy's own gradients (no fold-order and no exact-zero exception then); ``noise_of``: the gradients whose size scales
    the atomic noise when ``ref`` holds more than them (g0 + s: plus the two fp32 roundings of the sum)."""
    for n in pair.names:
        g, r = got[n], ref[n]
        if torch.equal(g, r):
            continue
        diff = float((g - r).abs().max())
        scale = float(r.abs().max())
        wn = n[:-4] + "weight"
        w_scale = float((noise_of or ref)[wn].abs().max()) if n.endswith(".bias") and wn in ref else 0.0
        print("[inplace] %s %s %s: max|diff| %.3e, max|ref| %.3e" % (pair.case, what, n, diff, scale))
        if n in pair.noisy:                      # behind a float-atomic sum: NOISY
            s_scale = float(noise_of[n].abs().max()) if noise_of is not None else scale
            if diff <= ATOMIC_BAR * max(s_scale, w_scale) + (2.0 ** -22 * scale if noise_of is not None else 0.0):
                continue
        elif not same_path:
            if (n in pair.loose or n in pair.linear_rows) and diff <= FOLD_BAR * scale:      # another FIXED order: _fold_order_params, LINEAR_ROWS
                continue
            if w_scale and not bool(g.any()) and scale <= 1e-4 * w_scale:
                continue        # exact 0 in place, autograd's rounding noise around 0 in the twin (tests/test_gpu_step.py:63)
        bad.append("%s: %s differs by %.3e (max|ref| %.3e)" % (what, n, diff, scale))


@pytest.fixture
def fresh_plans():
    stack.LAST_PLANS.clear()
    yield
    stack.LAST_PLANS.clear()


def _set_folds(monkeypatch, defer):
    monkeypatch.setattr(folds, "ENABLED", defer)


# ---- (a) one pass from zero, (b) it adds and only where it should, (c) micro-batches ----------------------------------------------------

@pytest.mark.parametrize("case,defer", [(c, True) for c in MODELS] + [(c, False) for c in STACK_MODELS])
def test_one_pass_accumulation_and_micro_batches_equal_the_twin(dev, case, defer, monkeypatch, fresh_plans):
    _set_folds(monkeypatch, defer)
    pair = Pair(case, dev)
    flat = pair.flat
    a1, a2 = pair.batch(dev, 21), pair.batch(dev, 22)
    bad = []
    # (a) one pass from zero
    pair.zero()
    pair.step(a1)
    s = pair.grads()
    _compare(pair, s, pair.twin_grads(), "(a) one pass from zero", bad)
    assert any(bool(g.any()) for g in s.values())
    gap = pair.gap_mask()
    assert bool(gap.any()) or case in NO_GAP, "no parameter of this model leaves a padding gap"
    assert not bool(flat.grad[gap].any()), "(a): a padding gap of flat.grad was written"
    # (b) it adds, and only where it should: all of flat.grad, gaps included, pre-filled with seeded random values
    g0 = torch.randn(flat.numel, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    flat.grad.copy_(g0)
    data0 = flat.data.clone()
    pair.step(a1, both=False)
    want = {}
    for p, off, n in zip(flat.params, flat._offsets, pair.names):
        # ONE fp32 add per element: every accumulate flavour ends in a single `*o + s` (folds.hip, fold.h) or `grad += s` (AccumulateGrad);
        # no node of these models adds into one element in more than one step, so the two-rounding allowance is taken only where s itself
        # is not reproducible (NOISY: s of this pass is another sum of the same terms)
        want[n] = g0[off: off + p.numel()].view(p.shape) + s[n]
    _compare(pair, pair.grads(), want, "(b) g0 + s", bad, same_path=True, noise_of=s)
    assert torch.equal(flat.grad[gap], g0[gap]), "(b): a padding gap of flat.grad lost its bits (a store past a parameter's end)"
    assert torch.equal(flat.data, data0), "(b): the backward wrote into flat.data"
    # (c) micro-batches: two different batches, backward after each, nothing zeroed in between
    pair.zero()
    pair.step(a1)
    pair.step(a2)
    _compare(pair, pair.grads(), pair.twin_grads(), "(c) two micro-batches", bad)
    assert not bool(flat.grad[gap].any()), "(c): a padding gap of flat.grad was written"
    pair.check_hooks()
    assert not bad, bad


# ---- (d) one module, two applications, one backward -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["sa_layer", "ssg_clas16", "pointnet_seg", "kdnet", "kdunet", "voxnet", "pfn"])
def test_one_module_applied_twice_in_one_backward_equals_the_twin(dev, case, fresh_plans):
    """loss = f(m(x1)) + f(m(x2)), ONE backward.  Both applications of a deferring stack queue accumulate jobs on the same .grad into the
    same fold list: the jobs must apply one after the other (papc_fold_jobs_f32 starts a new launch at an overlapping output).  sa_layer:
    a single set-abstraction layer, whose jobs all fit one launch; ssg_clas16: the whole classifier and the fused head; pointnet_seg: the
    point-wise stacks (planes path), linear_rows and the cloud-concat conv; kdnet / kdunet: kdconv, kdconv_bn (and linear_rows); voxnet: the
    voxconv backbone; pfn: the PFN layer.  Run twice: the step is meant to be reproducible (none of these models is in NOISY).
    The twin adds the two applications' gradients in autograd (s2 + s1), the flat copy as (0 + s2) + s1: the same bits."""
    pair = Pair(case, dev)
    a1, a2 = pair.batch(dev, 31), pair.batch(dev, 32)
    bad, runs = [], []
    for _ in range(2):
        pair.zero()
        (f1, o1), (f2, o2) = pair.loss(pair.model, a1), pair.loss(pair.model, a2)
        (t1, p1), (t2, p2) = pair.loss(pair.twin, a1), pair.loss(pair.twin, a2)
        assert torch.equal(o1.detach(), p1.detach()) and torch.equal(o2.detach(), p2.detach()), "the two forwards differ"
        (t1 + t2).backward()
        (f1 + f2).backward()
        torch.cuda.synchronize()
        if folds.ENABLED:
            pair.loose |= _fold_order_params(pair.model)
        runs.append(pair.grads())
        _compare(pair, runs[-1], pair.twin_grads(), "(d) two applications, one backward", bad)
    for n in pair.names:
        assert torch.equal(runs[0][n], runs[1][n]), "(d): %s differs between two identical runs" % n
    pair.check_hooks()
    assert not bad, bad


# ---- (e) a frozen subset ----------------------------------------------------------------------------------------------------------------

def _norm_params(m):
    return [n + "." + k for n, mod in m.named_modules() if "Norm" in type(mod).__name__ for k, _ in mod.named_parameters(recurse=False)]


def _first_child_params(m):
    """the first stack or backbone: the first child module that has parameters (PointNet_Basic_Clas keeps its one stack in two lists)"""
    if isinstance(m, PointNet_Basic_Clas):
        return [n for n, _ in m.named_parameters() if n.startswith(("convs.", "bns."))]
    name, child = next((n, c) for n, c in m.named_children() if any(True for _ in c.parameters()))
    return [name + "." + k for k, _ in child.named_parameters()]


def _one_conv_weight(m):
    return [next(n for n, p in m.named_parameters() if n.endswith("weight") and p.dim() >= 2)]


FREEZE = {"norms": _norm_params, "first": _first_child_params, "one_weight": _one_conv_weight}
# KDNet has no norm; the PFN layer's first child is the whole layer
FROZEN_CASES = [(c, g) for c in MODELS for g in FREEZE if (c, g) not in (("kdnet", "norms"), ("pfn", "first"))]


@pytest.mark.parametrize("case,group", FROZEN_CASES)
def test_frozen_subset_equals_the_twin_frozen_the_same_way(dev, case, group, fresh_plans):
    """requires_grad_(False) before FlatParams on (1) every norm's affine parameters, (2) the first stack or backbone, (3) one conv weight --
    the last leaves a PARTIAL target set, which nodeparts.all_or_none counts as none and nodeparts.LayerSlots splits (dW through autograd,
    dgamma / dbeta in place).  Trainable parameters equal a twin frozen the same way, frozen ones keep grad None, flat.grad holds no element
    for them and its gaps stay zero.  A node with a partial target set legitimately returns its gradients to autograd, so the hooks are held
    to VIA_AUTOGRAD only under (2), where every node left trainable has its full set."""
    pair = Pair(case, dev, freeze=FREEZE[group])
    assert pair.frozen and pair.names, (pair.frozen, pair.names)
    flat = pair.flat
    bad = []
    pair.zero()
    pair.step(pair.batch(dev, 41))
    _compare(pair, pair.grads(), pair.twin_grads(), "(e) frozen %s" % group, bad)
    for (n, p), (_, q) in zip(pair.model.named_parameters(), pair.twin.named_parameters()):
        if n in pair.frozen:
            assert p.grad is None and q.grad is None and not p.requires_grad, "frozen %s received a gradient" % n
    assert flat.numel == sum(p.numel() + (-p.numel()) % 4 for p in pair.model.parameters() if p.requires_grad)
    assert not bool(flat.grad[pair.gap_mask()].any()), "(e): a padding gap of flat.grad was written"
    print("[inplace] %s frozen %s: hooks fired for %s" % (case, group, sorted(set(pair.fired))))
    if group == "first":
        assert set(pair.fired) <= VIA_AUTOGRAD.get(case, set()), sorted(set(pair.fired))
    assert not bad, bad


# ---- (f) backward(retain_graph=True) twice on one graph -----------------------------------------------------------------------------------

@pytest.mark.parametrize("case", MODELS)
def test_second_backward_of_a_retained_graph_doubles_or_raises(dev, case, fresh_plans):
    """Either .grad is (0 + s) + s, bit for bit, or the second call raises PapcError before it launches anything (.grad still s).  (NOISY
    tensors: the second pass's s is another sum of the same terms.)  As the code stands no node writes into what its forward saved: every
    model takes the first branch."""
    pair = Pair(case, dev)
    pair.zero()
    loss, _ = pair.loss(pair.model, pair.batch(dev, 51))
    loss.backward(retain_graph=True)
    torch.cuda.synchronize()
    s = pair.grads()
    try:
        loss.backward(retain_graph=True)
        raised = False
    except _lib.PapcError:
        raised = True
    torch.cuda.synchronize()
    bad = []
    _compare(pair, pair.grads(), {n: (g if raised else g + g) for n, g in s.items()}, "(f) second backward (raised: %s)" % raised, bad,
             same_path=True, noise_of=s)
    pair.check_hooks()
    assert not bad, bad


# ---- (g) the fold list fills up -------------------------------------------------------------------------------------------------------------

def test_full_fold_list_lets_later_stacks_fold_on_their_own(dev, monkeypatch, fresh_plans):
    """folds.CAPACITY small enough that the SSG classifier's backward crosses CAPACITY - 16 part-way: the stacks behind that point get no list
    (folds.pending returns None) and fold on their own.  Gradients equal the default capacity's at FOLD_BAR for the tensors of
    _fold_order_params (their fold changes its kind), bit for bit elsewhere."""
    a = CASES["ssg_clas16"][1](dev, 61)
    res, answers = [], []
    inner = folds.pending

    def recording(keep):
        r = inner(keep)
        answers.append(r is not None)
        return r

    for cap in (folds.CAPACITY, 18):
        monkeypatch.setattr(folds, "CAPACITY", cap)
        monkeypatch.setattr(folds, "pending", recording)
        del answers[:]
        pair = Pair("ssg_clas16", dev)
        pair.zero()
        pair.step(a)
        res.append((pair, pair.grads(), list(answers)))
        pair.check_hooks()
        monkeypatch.setattr(folds, "pending", inner)
    (pair, g_all, ans_all), (_, g_few, ans_few) = res
    assert all(ans_all) and len(ans_all) >= 2, ans_all
    assert ans_few[0] and not ans_few[-1], "the list did not fill up part-way: %s" % ans_few
    bad = []
    _compare(pair, g_few, g_all, "(g) full list", bad)
    assert not bad, bad


# ---- a step without sharing still folds in ONE launch -----------------------------------------------------------------------------------

def _fold_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if "fold_jobs_kernel" in e.key)


def test_fold_launches_one_without_sharing_one_per_application_with(dev, fresh_plans):
    """papc_fold_jobs_f32 splits its launches only at overlapping outputs: the SSG classifier's step (whose gather-add first layer queues two
    interleaved column blocks of one dW) folds in ONE launch, the same model applied twice in one backward in two."""
    pair = Pair("ssg_clas16", dev)
    a1, a2 = pair.batch(dev, 71), pair.batch(dev, 72)
    pair.zero()
    pair.loss(pair.model, a1)[0].backward()              # (warm-up: lazily created streams and constants)
    torch.cuda.synchronize()
    assert _fold_launches(lambda: pair.loss(pair.model, a1)[0].backward()) == 1
    assert _fold_launches(lambda: (pair.loss(pair.model, a1)[0] + pair.loss(pair.model, a2)[0]).backward()) == 2
