"""GPU parity of the training-target stage (papc_amd.targets on csrc/dettarget.hip) with what the reference's own functions recorded
(tests/golden/ref_dettarget.npz; scenes and the comparison in tests/dettarget_cases.py).  Both flavours run on pre-poisoned output buffers:
integer outputs and the mask are compared exactly, max_overlap bit for bit -- which is what holds the device's division and operation order
to the source's -- and reg_targets within 1e-6 of the size of each element's own terms."""
import numpy as np
import pytest
import torch

from tests import dettarget_cases as C
from tests.util import assert_close

pytestmark = pytest.mark.gpu

ALL = sorted(C.SCENES)


def _cuda(x):
    return torch.from_numpy(np.array(x)).cuda()


def _poisoned(B, A, code):
    """output buffers pre-filled with NaN / a sentinel: every element must be written"""
    i32 = lambda *shape: torch.full(shape, -77, dtype=torch.int32, device="cuda")            # noqa: E731
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")                      # noqa: E731
    return {"labels": i32(B, A), "reg_targets": nan(B, A, code), "reg_weights": nan(B, A), "gt_ids": i32(B, A), "max_overlap": nan(B, A),
            "num_pos": i32(B)}


def _run(name, fused, cache=None, out=None, mask_out=None, workspaces=(None, None)):
    from papc_amd import targets as T
    s, g = C.golden(name)
    cache = C.make_cache(T, s, "cuda") if cache is None else cache
    B, A = g["mask"].shape
    mask_out = torch.full((B, A), 77, dtype=torch.uint8, device="cuda") if mask_out is None else mask_out
    mask = T.anchors_mask(_cuda(g["coors"]), B, cache, anchor_area_threshold=s["area_thr"], out=mask_out, workspace=workspaces[0], fused=fused)
    out = _poisoned(B, A, 8 if s["angle_vec"] else 7) if out is None else out
    got = T.assign(cache, _cuda(g["gt_boxes"]), _cuda(g["gt_classes"]), _cuda(g["num_gt"]), mask, out=out, workspace=workspaces[1], fused=fused)
    assert got is out and mask is mask_out
    return mask.cpu().numpy(), {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ALL)
def test_scene_against_the_reference(name, fused):
    s, g = C.golden(name)
    mask, got = _run(name, fused)
    assert np.array_equal(mask, g["mask"]), name
    C.check_assign(got, g, s, ("fused " if fused else "torch ") + name)


def test_cache_on_the_device_holds_the_references_anchors():
    from papc_amd import targets as T
    s, g = C.golden("e")
    cache = C.make_cache(T, s, "cuda")
    assert all(cache[k].is_cuda for k in ("anchors", "anchors_bv", "cells", "matched_thresholds", "unmatched_thresholds"))
    assert np.array_equal(C.bits(cache["anchors_bv"].cpu().numpy()), C.bits(g["anchors_bv"])) and np.array_equal(cache["cells"].cpu().numpy(), g["cells"])


@pytest.mark.parametrize("name", ["c", "d"])
def test_two_runs_are_bit_identical(name):
    m1, r1 = _run(name, True)
    m2, r2 = _run(name, True)
    assert np.array_equal(m1, m2) and all(np.array_equal(C.bits(r1[k]), C.bits(r2[k])) for k in r1)


def test_without_a_mask_every_anchor_is_inside():
    """anchors_mask=None against an all-ones mask, and against the torch-op flavour"""
    from papc_amd import targets as T
    s, g = C.golden("b")
    cache = C.make_cache(T, s, "cuda")
    gt = (_cuda(g["gt_boxes"]), _cuda(g["gt_classes"]), _cuda(g["num_gt"]))
    A = g["mask"].shape[1]
    none = T.assign(cache, *gt, None, out=_poisoned(1, A, 7), fused=True)
    ones = T.assign(cache, *gt, torch.ones(1, A, dtype=torch.uint8, device="cuda"), out=_poisoned(1, A, 7), fused=True)
    ref = T.assign(cache, *gt, None, fused=False)
    for k in none:
        assert torch.equal(none[k], ones[k]), k
        if k != "reg_targets":
            assert torch.equal(none[k], ref[k]), k
    assert (none["max_overlap"] == 1.0).sum() == 2                      # both gts that sit exactly on an anchor find it now
    assert_close(none["reg_targets"].cpu().numpy(), ref["reg_targets"].cpu().numpy(), rel=1e-6, what="reg_targets without a mask")


def test_workspace_and_out_reuse():
    from papc_amd import targets as T
    s, g = C.golden("c")
    B, A = g["mask"].shape
    cache = C.make_cache(T, s, "cuda")
    ws = (torch.empty(T.mask_workspace_bytes(B, A, 42, 38) + 512, dtype=torch.uint8, device="cuda"),
          torch.empty(T.assign_workspace_bytes(B, A, 33) + 512, dtype=torch.uint8, device="cuda"))
    out, mask_out = _poisoned(B, A, 7), torch.full((B, A), 77, dtype=torch.uint8, device="cuda")
    for _ in range(2):                                                   # the second call finds the first one's results in every buffer
        mask, got = _run("c", True, cache=cache, out=out, mask_out=mask_out, workspaces=ws)
        assert np.array_equal(mask, g["mask"])
        C.check_assign(got, g, s, "reuse c")
    with pytest.raises(AssertionError, match="workspace"):
        T.anchors_mask(_cuda(g["coors"]), B, cache, workspace=ws[0][:64], fused=True)
    with pytest.raises(AssertionError, match="workspace"):
        T.assign(cache, _cuda(g["gt_boxes"]), _cuda(g["gt_classes"]), _cuda(g["num_gt"]), workspace=ws[1][:64], fused=True)


@pytest.mark.parametrize("angle_vec", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
def test_encode_and_decode_round_trip(smooth, angle_vec):
    from papc_amd import detect, targets as T
    _, g = C.golden("c")
    boxes = _cuda(g["gt_boxes"][0])                                      # 33 boxes against the first 33 anchors: offsets of metres
    anchors = _cuda(g["anchors"].reshape(-1, 7)[:33])
    enc = T.second_box_encode(boxes, anchors, angle_vec, smooth, fused=True)
    assert enc.shape == (33, 8 if angle_vec else 7)
    assert_close(enc.cpu().numpy(), T.second_box_encode(boxes.cpu(), anchors.cpu(), angle_vec, smooth, fused=False).numpy(), rel=1e-6,
                 what="second_box_encode against the torch-op flavour")
    back = detect.second_box_decode(enc, anchors, angle_vec, smooth, fused=True).cpu().numpy()
    want = g["gt_boxes"][0].astype(np.float64)
    if angle_vec:                                                        # atan2 gives the angle in (-pi, pi]
        want[:, 6] = np.arctan2(np.sin(want[:, 6]), np.cos(want[:, 6]))
    assert np.abs(back - want).max() <= 2e-5, np.abs(back - want).max()  # coordinates of up to 16 m through a difference and a sum in fp32


def test_end_to_end_mask_assign_loss_predict():
    """scene (c): anchors_mask -> assign -> detloss.pointpillars_loss gives the loss and the three gradients that the recorded targets give, and
    detect.predict_tensors takes the produced mask as it is"""
    from papc_amd import detect, detloss, targets as T
    s, g = C.golden("c")
    B, A = g["mask"].shape
    cache = C.make_cache(T, s, "cuda")
    mask = T.anchors_mask(_cuda(g["coors"]), B, cache, anchor_area_threshold=s["area_thr"], fused=True)
    tg = T.assign(cache, _cuda(g["gt_boxes"]), _cuda(g["gt_classes"]), _cuda(g["num_gt"]), mask, fused=True)
    gen = torch.Generator().manual_seed(3)
    preds = [torch.randn((B, A, c), generator=gen).mul_(0.3).cuda() for c in (7, 2, 2)]
    anchors = cache["anchors"][None].expand(B, A, 7).contiguous()

    def loss_and_grads(labels, reg_targets):
        leaves = [p.clone().requires_grad_(True) for p in preds]
        r = detloss.pointpillars_loss(*leaves, labels, reg_targets, anchors, num_class=2, fused=True)
        r["loss"].backward()
        return [r["loss"].detach().cpu().numpy()] + [p.grad.cpu().numpy() for p in leaves]

    got = loss_and_grads(tg["labels"], tg["reg_targets"])
    want = loss_and_grads(_cuda(g["labels"]), _cuda(g["reg_targets"]))
    for x, y, what in zip(got, want, ("loss", "d box_preds", "d cls_preds", "d dir_cls_preds")):
        assert np.isfinite(x).all() and np.abs(y).max() > 0, what
        assert_close(x, y, rel=1e-5, what="end to end " + what)

    kw = dict(num_class=2, nms_score_threshold=0.05, nms_pre_max_size=100, nms_post_max_size=30, nms_iou_threshold=0.5, fused=True)
    r1 = detect.predict_tensors(*preds, cache["anchors"], mask, **kw)
    r2 = detect.predict_tensors(*preds, cache["anchors"], _cuda(g["mask"]), **kw)
    assert all(torch.equal(r1[k], r2[k]) for k in r1) and int(r1["num_det"][2]) == 0 and int(r1["num_det"][0]) > 0
