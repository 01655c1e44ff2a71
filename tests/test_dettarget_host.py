"""CPU checks of the training-target stage (papc_amd.targets on csrc/dettarget.hip): the torch-op flavour on CPU tensors against what the
reference's own functions recorded (tests/golden/ref_dettarget.npz, scenes in tests/dettarget_cases.py), one case worked by hand, the struct
mirrors and the argument validation of the C entry points."""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib
from tests import dettarget_cases as C

ALL = sorted(C.SCENES)


def _t(x):
    return torch.from_numpy(np.array(x))


@pytest.mark.parametrize("name", ALL)
def test_anchors_and_cells_against_the_reference(name):
    from papc_amd import targets as T
    s, g = C.golden(name)
    ret = C.make_assigner(T, s).generate_anchors(s["fmap"])
    assert ret["anchors"].shape == g["anchors"].shape and ret["anchors"].dtype == np.float32
    for k in ("anchors", "matched_thresholds", "unmatched_thresholds"):
        assert np.array_equal(C.bits(ret[k]), C.bits(g[k])), (name, k)
    cache = C.make_cache(T, s, "cpu")
    assert np.array_equal(C.bits(cache["anchors"].numpy()), C.bits(g["anchors"].reshape(-1, 7)))
    assert np.array_equal(C.bits(cache["anchors_bv"].numpy()), C.bits(g["anchors_bv"])), name
    assert cache["cells"].dtype == torch.int32 and np.array_equal(cache["cells"].numpy(), g["cells"]), name


def test_threshold_vectors_keep_the_sources_order():
    """two generators: anchors interleave per location (axis -2), the threshold vectors do not (axis 0)"""
    from papc_amd import targets as T
    s, g = C.golden("e")
    ret = C.make_assigner(T, s).generate_anchors(s["fmap"])
    A = ret["matched_thresholds"].shape[0]
    assert ret["anchors"].shape == (1, 10, 9, 4, 7) and A == 360
    assert (ret["matched_thresholds"][:A // 2] == np.float32(0.6)).all() and (ret["matched_thresholds"][A // 2:] == np.float32(0.5)).all()
    sizes = ret["anchors"].reshape(-1, 7)[:, 3]
    assert (sizes[:4] == np.array([1.6, 1.6, 0.6, 0.6], np.float32)).all()


@pytest.mark.parametrize("name", ALL)
def test_torch_flavour_on_cpu_reproduces_the_reference(name):
    from papc_amd import targets as T
    s, g = C.golden(name)
    cache = C.make_cache(T, s, "cpu")
    B = g["num_gt"].shape[0]
    mask = T.anchors_mask(_t(g["coors"]), B, cache, anchor_area_threshold=s["area_thr"], fused=False)
    assert mask.dtype == torch.uint8 and np.array_equal(mask.numpy(), g["mask"]), name
    got = T.assign(cache, _t(g["gt_boxes"]), _t(g["gt_classes"]), _t(g["num_gt"]), mask, fused=False)
    C.check_assign({k: v.numpy() for k, v in got.items()}, g, s, "cpu " + name)


@pytest.mark.parametrize("angle_vec", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
def test_second_box_encode_inverts_the_decode_on_cpu(smooth, angle_vec):
    from papc_amd import detect, targets as T
    _, g = C.golden("a")
    anchors = _t(g["anchors"].reshape(-1, 7)[:5])
    boxes = _t(g["gt_boxes"][0])
    enc = T.second_box_encode(boxes, anchors, angle_vec, smooth, fused=False)
    assert enc.shape == (5, 8 if angle_vec else 7)
    back = detect.second_box_decode(enc, anchors, angle_vec, smooth, fused=False)
    want = boxes.clone()
    if angle_vec:                                                        # atan2 gives the angle in (-pi, pi]
        want[:, 6] = torch.atan2(torch.sin(want[:, 6]), torch.cos(want[:, 6]))
    assert torch.allclose(back, want, rtol=0, atol=2e-5)


def test_two_anchors_two_gts_by_hand():
    """a0 = (0, 0) and a1 = (3, 0), both 2 x 4 at angle 0: near-bboxes (-1, -2, 1, 2) and (2, -2, 4, 2), area 8.
    g0 = (0.5, 0), 2 x 4, class 1 -> (-0.5, -2, 1.5, 2): with a0 iw = 1 - (-0.5) = 1.5, ih = 4, ua = 8 + 8 - 6 = 10, IoU 0.6; with a1 iw < 0 -> 0.
    g1 = (3, 1), 2 x 2, class 2 -> (2, 0, 4, 2), area 4: with a1 iw = 2, ih = 2, ua = 8 + 4 - 4 = 8, IoU 0.5; with a0 iw < 0 -> 0.
    a0: amax 0.6 >= matched 0.6 (and it holds g0's maximum): label 1, gt 0; x target 0.5 / sqrt(4^2 + 2^2) = 0.1118034, the rest 0.
    a1: amax 0.5 lies between unmatched 0.45 and matched 0.6 -- don't care by the thresholds -- but it holds g1's maximum: forced, label 2, gt 1;
        y target 1 / sqrt(20) = 0.2236068, length target log(2 / 4) = -0.6931472, the rest 0.
    With a1 masked out g1 overlaps no inside anchor (gmax 0 -> -1) and forces nothing: a1 is -1 with zeros, a0 unchanged."""
    from papc_amd import targets as T
    anchors = torch.tensor([[0, 0, -1, 2, 4, 1.5, 0], [3, 0, -1, 2, 4, 1.5, 0]], dtype=torch.float32)
    cache = {"anchors": anchors, "anchors_bv": T.rbbox2d_to_near_bbox(anchors[:, [0, 1, 3, 4, 6]]), "matched_thresholds": torch.full((2,), 0.6),
             "unmatched_thresholds": torch.full((2,), 0.45), "encode_angle_to_vector": False, "smooth_dim": False, "positive_fraction": None}
    assert cache["anchors_bv"].tolist() == [[-1, -2, 1, 2], [2, -2, 4, 2]]
    gt = torch.tensor([[[0.5, 0, -1, 2, 4, 1.5, 0], [3, 1, -1, 2, 2, 1.5, 0]]], dtype=torch.float32)
    cls, n = torch.tensor([[1, 2]], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    r = T.assign(cache, gt, cls, n, fused=False)
    assert r["labels"].tolist() == [[1, 2]] and r["gt_ids"].tolist() == [[0, 1]] and r["num_pos"].tolist() == [2]
    assert r["max_overlap"].tolist() == [[float(np.float32(0.6)), 0.5]] and r["reg_weights"].tolist() == [[1.0, 1.0]]
    want = np.zeros((1, 2, 7))
    want[0, 0, 0], want[0, 1, 1], want[0, 1, 4] = 0.5 / np.sqrt(20.0), 1.0 / np.sqrt(20.0), np.log(0.5)
    assert np.abs(r["reg_targets"].numpy() - want).max() < 1e-6
    r = T.assign(cache, gt, cls, n, torch.tensor([[1, 0]], dtype=torch.uint8), fused=False)
    assert r["labels"].tolist() == [[1, -1]] and r["gt_ids"].tolist() == [[0, -1]] and r["num_pos"].tolist() == [1]
    assert r["max_overlap"].tolist() == [[float(np.float32(0.6)), 0.0]] and (r["reg_targets"][0, 1] == 0).all() and r["reg_weights"].tolist() == [[1.0, 0.0]]


def test_cells_outside_the_grid_are_refused():
    from papc_amd import targets as T
    bv = np.array([[-5.0, 0.0, -3.0, 1.0]], np.float32)                  # wholly left of the grid: x2 < 0 after the one-sided clamps
    with pytest.raises(_lib.PapcError):
        T.anchor_cells(bv, [0.5, 0.5, 4.0], [0.0, 0.0, -3.0, 8.0, 8.0, 1.0], (16, 16, 1))
    bv = np.array([[9.0, 0.0, 11.0, 1.0]], np.float32)                   # wholly right of it: x1 > nx - 1
    with pytest.raises(_lib.PapcError):
        T.anchor_cells(bv, [0.5, 0.5, 4.0], [0.0, 0.0, -3.0, 8.0, 8.0, 1.0], (16, 16, 1))


def test_struct_mirrors_match_the_library():
    from papc_amd import targets as T
    lib = _lib.load()
    for cls, cname in ((T.AnchorsMaskDesc, b"papc_anchors_mask_desc"), (T.AnchorsMaskIo, b"papc_anchors_mask_io"),
                       (T.DetAssignDesc, b"papc_det_assign_desc"), (T.DetAssignIo, b"papc_det_assign_io")):
        assert ctypes.sizeof(cls) == lib.papc_abi_sizeof(cname) > 0, cname


def test_argument_validation_without_gpu():
    """every limit is refused on the host, before any launch, with -1 (or (size_t)-1) and a message"""
    from papc_amd import targets as T
    lib = _lib.load()
    bad = ctypes.c_size_t(-1).value
    err = lambda: lib.papc_last_error_string().decode()                 # noqa: E731
    ws = ctypes.create_string_buffer(1 << 16)
    good = dict(B=2, A=100, Gmax=8, encode_angle_to_vector=0, smooth_dim=0, code_size=7)
    assert lib.papc_det_assign_workspace(ctypes.byref(T.DetAssignDesc(**good))) not in (0, bad)
    for over, word in ((dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(A=0), "A=0"), (dict(B=65535, A=40000), "2^31"),
                       (dict(Gmax=257), "Gmax=257"), (dict(Gmax=-1), "Gmax=-1"), (dict(code_size=8), "code_size=8"),
                       (dict(encode_angle_to_vector=1), "code_size=7")):
        d = T.DetAssignDesc(**dict(good, **over))
        assert lib.papc_det_assign_workspace(ctypes.byref(d)) == bad and word in err(), (over, err())
        assert lib.papc_det_assign_f32(ctypes.byref(d), ctypes.byref(T.DetAssignIo()), ws, len(ws), None) == -1 and word in err(), (over, err())
    assert lib.papc_det_assign_workspace(None) == bad and "null" in err()
    d = T.DetAssignDesc(**good)
    assert lib.papc_det_assign_f32(ctypes.byref(d), None, ws, len(ws), None) == -1 and "null" in err()
    assert lib.papc_det_assign_f32(ctypes.byref(d), ctypes.byref(T.DetAssignIo()), None, 0, None) == -1 and "null" in err()
    assert lib.papc_det_assign_f32(ctypes.byref(d), ctypes.byref(T.DetAssignIo()), ws, len(ws), None) == -1 and "null input" in err()
    p = ctypes.addressof(ws)
    io = T.DetAssignIo(anchors=p, anchors_bv=p, matched=p, unmatched=p, gt_boxes=p, gt_classes=p, num_gt=p)
    assert lib.papc_det_assign_f32(ctypes.byref(d), ctypes.byref(io), ws, len(ws), None) == -1 and "null output" in err()
    io = T.DetAssignIo(anchors=p, anchors_bv=p, matched=p, unmatched=p, gt_boxes=p, gt_classes=p, num_gt=p, labels=p, reg_targets=p, reg_weights=p)
    assert lib.papc_det_assign_f32(ctypes.byref(d), ctypes.byref(io), ws, 16, None) == -1 and "workspace too small" in err()

    good = dict(B=2, A=100, ny=16, nx=16, P=10, area_thresh=1.0)
    assert lib.papc_anchors_mask_workspace(ctypes.byref(T.AnchorsMaskDesc(**good))) not in (0, bad)
    for over, word in ((dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(A=0), "A=0"), (dict(B=65535, A=40000), "2^31"), (dict(ny=0), "ny=0"),
                       (dict(nx=0), "nx=0"), (dict(ny=1 << 16, nx=1 << 16), "2^31"), (dict(P=-1), "P=-1")):
        d = T.AnchorsMaskDesc(**dict(good, **over))
        assert lib.papc_anchors_mask_workspace(ctypes.byref(d)) == bad and word in err(), (over, err())
        assert lib.papc_anchors_mask_u8(ctypes.byref(d), ctypes.byref(T.AnchorsMaskIo()), ws, len(ws), None) == -1 and word in err(), (over, err())
    d = T.AnchorsMaskDesc(**good)
    assert lib.papc_anchors_mask_u8(ctypes.byref(d), None, ws, len(ws), None) == -1 and "null" in err()
    assert lib.papc_anchors_mask_u8(ctypes.byref(d), ctypes.byref(T.AnchorsMaskIo()), ws, len(ws), None) == -1 and "null input" in err()
    assert lib.papc_anchors_mask_u8(ctypes.byref(d), ctypes.byref(T.AnchorsMaskIo(coors=p, cells=p)), ws, len(ws), None) == -1 and "null output" in err()
    assert lib.papc_anchors_mask_u8(ctypes.byref(d), ctypes.byref(T.AnchorsMaskIo(coors=p, cells=p, mask=p)), ws, 16, None) == -1
    assert "workspace too small" in err()

    assert lib.papc_box_encode_f32(None, None, 1, 7, 0, 0, None, None) == -1 and "null" in err()
    assert lib.papc_box_encode_f32(p, p, 0, 7, 0, 0, p, None) == -1 and "n=0" in err()
    assert lib.papc_box_encode_f32(p, p, 1, 7, 1, 0, p, None) == -1 and "code_size=7" in err()
    with pytest.raises(_lib.PapcError):
        T.assign_workspace_bytes(1, 10, 257)
    with pytest.raises(_lib.PapcError):
        T.mask_workspace_bytes(1, 10, 0, 4)


def test_no_cpu_fallback_and_no_sampling_path():
    from papc_amd import targets as T
    s, g = C.golden("a")
    cache = C.make_cache(T, s, "cpu")
    gt = (_t(g["gt_boxes"]), _t(g["gt_classes"]), _t(g["num_gt"]))
    with pytest.raises(_lib.PapcError):
        T.anchors_mask(_t(g["coors"]), 1, cache, fused=True)
    with pytest.raises(_lib.PapcError):
        T.assign(cache, *gt, fused=True)
    with pytest.raises(_lib.PapcError):
        T.second_box_encode(gt[0][0], cache["anchors"][:5], fused=True)
    sampled = T.anchor_cache(C.make_assigner(T, s, positive_fraction=0.5), s["fmap"], s["voxel_size"], s["pc_range"], s["grid_size"], device="cpu")
    for fused in (False, True):
        with pytest.raises(_lib.PapcError, match="positive_fraction"):
            T.assign(sampled, *gt, fused=fused)
    with pytest.raises(_lib.PapcError, match="Gmax"):
        T.assign(cache, torch.zeros(1, 257, 7), torch.ones(1, 257, dtype=torch.int32), torch.tensor([1], dtype=torch.int32), fused=False)
