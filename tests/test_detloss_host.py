"""Host checks of the PointPillars detection loss (papc_amd/detloss.py, csrc/detloss.hip): the float64 restatement against a case worked
by hand, the ABI of the two new structs, argument validation before any launch, the flavour switch, and the torch-op flavour on CPU tensors.

The case worked by hand (test_reference_reproduces_the_hand_worked_case): B = 1, A = 2, C = 1, NormByNumPositives, pos / neg class weight 1,
alpha 0.25, gamma 2, sigma 3 (knee 1/9), unit code weights, no sin-difference, loc / cls / direction weights 2 / 1 / 0.2.
  anchor 0: label 1 (positive); anchor 1: label -1 (don't care).  numpos = 1, so cls_weights = (1 + [pos]) / 1 = (2, 1) -- the don't-care
  anchor keeps neg_cls_weight (:480) -- and reg_weights = (1, 0).
  cls logits (0, 0): cross-entropy ln 2, (1 - p_t)^2 = 1/4 at both.  anchor 0 (target 1): 1/4 * 0.25 * ln 2 * 2 = 0.125 ln 2;
    anchor 1 (target 0 after the cared mask): 1/4 * 0.75 * ln 2 * 1 = 0.1875 ln 2.  cls_loss_reduced = 0.3125 ln 2 = 0.2166085;
    cls_pos_loss = 0.125 ln 2 = 0.0866434; cls_neg_loss = 0: anchor 1 is not a negative.
  box diffs of anchor 0: (0.0625, 1, 0, 0, 0, 0, 0).  0.0625 <= 1/9: 0.5 (0.0625 * 3)^2 = 0.0175781; 1 > 1/9: 1 - 1/18 = 0.9444444; anchor 1's
    large diffs carry weight 0.  loc_loss_reduced = 2 * 0.9620226 = 1.9240451.
  direction: anchor 0 has reg_target 0 + anchor 0.5 > 0: class 1; logits (0, 0): ln 2 at weight 1/1.  dir_loss_reduced = 0.6931472.
  loss = 1.9240451 + 0.2166085 + 0.2 * 0.6931472 = 2.2792830.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import detloss as D
from tests import detloss_ref as R

E_INVALID, E_UNSUPPORTED = -1, -2          # include/papc_hip.h


def _hand_case():
    box = torch.tensor([[[0.0625, 1, 0, 0, 0, 0, 0], [5, -5, 5, -5, 5, -5, 5]]], dtype=torch.float32)
    cls = torch.zeros(1, 2, 1)
    dirp = torch.zeros(1, 2, 2)
    labels = torch.tensor([[1, -1]])
    tgt = torch.zeros(1, 2, 7)
    anchors = torch.zeros(1, 2, 7)
    anchors[0, :, 6] = 0.5
    kw = dict(num_class=1, loss_norm_type="NormByNumPositives", alpha=0.25, gamma=2.0, sigma=3.0, loc_weight=2.0, cls_weight=1.0,
              direction_loss_weight=0.2)
    return (box, cls, dirp, labels, tgt, anchors), kw


def test_reference_reproduces_the_hand_worked_case():
    (box, cls, dirp, labels, tgt, anchors), kw = _hand_case()
    r = R.pointpillars_loss(box.double(), cls.double(), dirp.double(), labels, tgt, anchors, **kw)
    ln2 = math.log(2.0)
    assert abs(float(r["cls_loss_reduced"]) - 0.3125 * ln2) < 1e-12
    assert abs(float(r["cls_pos_loss"]) - 0.125 * ln2) < 1e-12 and float(r["cls_neg_loss"]) == 0.0
    assert abs(float(r["loc_loss_reduced"]) - 2 * (0.017578125 + 1 - 1 / 18)) < 1e-12
    assert abs(float(r["dir_loss_reduced"]) - ln2) < 1e-12
    assert abs(float(r["loss"]) - 2.2792830) < 1e-6
    np.testing.assert_allclose(r["cls_loss"].numpy().ravel(), [0.125 * ln2, 0.1875 * ln2], rtol=1e-12)
    np.testing.assert_allclose(r["loc_loss"].numpy()[0, 0, :2], [0.017578125, 1 - 1 / 18], rtol=1e-12)
    assert float(r["loc_loss"][0, 1].abs().max()) == 0.0
    assert r["cared"].tolist() == [[True, False]] and r["dir_targets"].tolist() == [[1, 1]]


def test_struct_mirrors_and_abi_version():
    lib = _lib.load()
    assert lib.papc_abi_version() == 8
    assert ctypes.sizeof(D.DetLossDesc) == lib.papc_abi_sizeof(b"papc_det_loss_desc") > 0
    assert ctypes.sizeof(D.DetLossIo) == lib.papc_abi_sizeof(b"papc_det_loss_io") > 0


def test_switch_defaults_to_the_fused_node():
    assert D.fused_enabled() == (os.environ.get("PAPC_DET_LOSS", "1") != "0")


def _desc(**kw):
    d = D.DetLossDesc()
    d.B, d.A, d.C, d.code_size, d.norm_type, d.has_dir = 2, 65, 1, 7, 1, 1
    d.encode_background_as_zeros, d.codewise, d.sigma, d.gamma = 1, 1, 3.0, 2.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _message():
    return _lib.load().papc_last_error_string().decode()


@pytest.mark.parametrize("field,value,code,word", [
    ("C", 9, E_UNSUPPORTED, "C=9"), ("code_size", 8, E_UNSUPPORTED, "code size 8"),
    ("encode_background_as_zeros", 0, E_UNSUPPORTED, "encode_background_as_zeros"), ("codewise", 0, E_UNSUPPORTED, "codewise"),
    ("B", 0, E_INVALID, "B=0"), ("A", 0, E_INVALID, "A=0"), ("C", 0, E_INVALID, "C=0"), ("norm_type", 3, E_INVALID, "norm_type=3"),
    ("sigma", 0.0, E_INVALID, "sigma")])
def test_bad_descriptors_are_refused_with_a_message(field, value, code, word):
    """unsupported arguments: PAPC_E_UNSUPPORTED, bad sizes: PAPC_E_INVALID -- by both entry points, before anything is launched"""
    lib, d, n = _lib.load(), _desc(**{field: value}), ctypes.c_int64(0)
    assert lib.papc_det_loss_workspace(ctypes.byref(d), ctypes.byref(n)) == code
    assert word in _message()
    assert lib.papc_det_loss_fwd_f32(ctypes.byref(d), ctypes.byref(D.DetLossIo()), None) == code
    assert word in _message()


def test_null_arguments_are_refused_with_a_message():
    lib, d, n = _lib.load(), _desc(), ctypes.c_int64(0)
    assert lib.papc_det_loss_workspace(None, ctypes.byref(n)) == E_INVALID and "null" in _message()
    assert lib.papc_det_loss_workspace(ctypes.byref(d), None) == E_INVALID and "null" in _message()
    assert lib.papc_det_loss_workspace(ctypes.byref(d), ctypes.byref(n)) == 0 and n.value > 0
    assert lib.papc_det_loss_fwd_f32(None, ctypes.byref(D.DetLossIo()), None) == E_INVALID and "null" in _message()
    assert lib.papc_det_loss_fwd_f32(ctypes.byref(d), None, None) == E_INVALID and "null" in _message()
    required = ["box_preds", "cls_preds", "dir_preds", "labels", "reg_targets", "anchors", "out", "dbox", "dcls", "ddir", "workspace"]
    for missing in required:          # every other pointer looks valid: the null one alone must stop the call before a launch
        io = D.DetLossIo()
        for f in required:
            setattr(io, f, None if f == missing else 0x10000)
        assert lib.papc_det_loss_fwd_f32(ctypes.byref(d), ctypes.byref(io), None) == E_INVALID, missing
        assert "null" in _message(), missing
    io = D.DetLossIo()
    for f in required:
        setattr(io, f, 0x10004 if f == "ddir" else 0x10000)
    assert lib.papc_det_loss_fwd_f32(ctypes.byref(d), ctypes.byref(io), None) == E_INVALID and "aligned" in _message()


def test_no_cpu_fallback_of_the_fused_node():
    args, kw = _hand_case()
    with pytest.raises(_lib.PapcError):
        D.pointpillars_loss(*args, fused=True, **kw)


def _random_case(seed, B, A, C):
    g = torch.Generator().manual_seed(seed)
    box = torch.randn(B, A, 7, generator=g)
    tgt = box + 0.3 * torch.randn(B, A, 7, generator=g)
    cls = 3 * torch.randn(B, A, C, generator=g)
    dirp = torch.randn(B, A, 2, generator=g)
    labels = torch.randint(-1, C + 1, (B, A), generator=g)
    anchors = torch.randn(B, A, 7, generator=g)
    return box, cls, dirp, labels, tgt, anchors


def _close(got, ref, what, tol=1e-5):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), what
    bound = tol * (np.abs(ref) + np.abs(ref).max())
    err = np.abs(got - ref)
    assert (err <= bound).all(), "%s: max error %.3e at bound %.3e" % (what, err.max(), bound.flat[err.argmax()])


@pytest.mark.parametrize("norm", ["NormByNumExamples", "NormByNumPositives", "NormByNumPosNeg"])
@pytest.mark.parametrize("C,alpha,gamma,sin_diff", [(1, 0.25, 2.0, False), (3, 0.25, 1.5, True), (1, None, 0.0, True)])
def test_torch_op_flavour_on_cpu_matches_the_reference(norm, C, alpha, gamma, sin_diff):
    box, cls, dirp, labels, tgt, anchors = _random_case(3, 2, 65, C)
    cw = (1.0, 0.5, 2.0, 1.0, 1.5, 1.0, 0.75)
    kw = dict(num_class=C, loss_norm_type=norm, alpha=alpha, gamma=gamma, encode_rad_error_by_sin=sin_diff, code_weights=cw,
              pos_cls_weight=1.5, neg_cls_weight=0.5)
    leaves = [t.clone().requires_grad_() for t in (box, cls, dirp)]
    got = D.pointpillars_loss(*leaves, labels, tgt, anchors, fused=False, **kw)
    (got["loss"] * 0.7).backward()
    leaves64 = [t.double().requires_grad_() for t in (box, cls, dirp)]
    ref = R.pointpillars_loss(*leaves64, labels, tgt, anchors, **kw)
    (ref["loss"] * 0.7).backward()
    for k in ("loss", "cls_loss", "loc_loss", "cls_pos_loss", "cls_neg_loss", "dir_loss_reduced", "cls_loss_reduced", "loc_loss_reduced"):
        _close(got[k].detach().numpy(), ref[k].detach().numpy(), k)
    assert torch.equal(got["cared"], ref["cared"]) and got["cls_preds"] is leaves[1]
    for name, a, b in zip(("d box_preds", "d cls_preds", "d dir_preds"), leaves, leaves64):
        _close(a.grad.numpy(), b.grad.numpy(), name)
