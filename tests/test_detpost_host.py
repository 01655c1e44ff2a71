"""CPU checks of the predict() stage (papc_amd.detect, csrc/detpost.hip): the float64 restatement against a case worked by hand, the margin
condition that makes the GPU tests' exact comparisons legitimate, the struct mirrors, and the host-side argument checks (no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import detect
from tests import detpost_ref as D


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def test_restatement_on_a_case_worked_by_hand():
    """Four anchors, zero encodings (exp(0) = 1 and za + ha/2 - hg/2 = za: a decoded box IS its anchor), threshold 0.5, IoU threshold 0.5:
      0: logit 2  -> 0.8808, r = +0.3, dir (1, 0) -> dir label 0: (r > 0) xor 0 -> r + pi
      1: logit 0  -> exactly 0.5: ``>=`` keeps it; far away, r = -0.2, dir (0, 1) -> dir label 1: (r > 0) = False xor 1 -> r + pi
      2: logit -1 -> 0.2689: fails
      3: logit 1  -> 0.7311, anchor 0's box shifted by 0.1 m: passes, ranks second, suppressed by anchor 0 (IoU about 0.9)
    so 3 pass, and the detections are anchors 0 and 1 in that order."""
    anchors = np.array([[0.0, 0.0, -1.0, 2.0, 4.0, 1.5, 0.3],
                        [20.0, 0.0, -1.0, 2.0, 4.0, 1.5, -0.2],
                        [40.0, 0.0, -1.0, 2.0, 4.0, 1.5, 0.0],
                        [0.1, 0.0, -1.0, 2.0, 4.0, 1.5, 0.3]], np.float32)
    fr = dict(box=np.zeros((4, 7), np.float32), cls=np.array([[2.0], [0.0], [-1.0], [1.0]], np.float32),
              dir=np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [0.5, 0.5]], np.float32), anchors=anchors, mask=None)
    for rotate in (True, False):
        cfg = dict(D.CFG, rotate=rotate, score_thresh=0.5, pre_max=4, post_max=4)
        r = D.predict_frame(fr, cfg)
        assert r["num_pass"] == 3 and r["num_det"] == 2
        assert r["anchor_idx"].tolist() == [0, 1] and r["labels"].tolist() == [0, 0] and r["dir_labels"].tolist() == [0, 1]
        np.testing.assert_allclose(r["scores"], [_sig(2.0), 0.5], rtol=1e-15)
        want = anchors[[0, 1]].astype(np.float64)
        want[:, 6] += np.float64(np.float32(np.pi))
        np.testing.assert_allclose(r["boxes"], want, rtol=1e-12)
    r = D.predict_frame(fr, dict(D.CFG, rotate=True, score_thresh=0.5, pre_max=2, post_max=4))     # the top-k cut drops anchor 1 before the NMS
    assert r["num_pass"] == 3 and r["anchor_idx"].tolist() == [0]
    r = D.predict_frame(fr, dict(D.CFG, rotate=True, score_thresh=0.5, pre_max=4, post_max=1))
    assert r["anchor_idx"].tolist() == [0]


def test_decode_restatement_inverts_the_encoding_by_hand():
    """one box by hand: anchor (1, 2, -1, 2, 4, 1.5, 0.5), encoding (0.5, -0.5, 1, ln 2, ln 0.5, 0, 0.25): diagonal = sqrt(20), x = 1 + 0.5 sqrt(20),
    y = 2 - 0.5 sqrt(20), w = 4, l = 2, h = 1.5, z: (1 * 1.5 + (-1 + 0.75)) - 0.75 = 0.5, r = 0.75"""
    a = np.array([1.0, 2.0, -1.0, 2.0, 4.0, 1.5, 0.5])
    t = np.array([0.5, -0.5, 1.0, np.log(2.0), np.log(0.5), 0.0, 0.25])
    np.testing.assert_allclose(D.decode(t, a), [1 + 0.5 * np.sqrt(20.0), 2 - 0.5 * np.sqrt(20.0), 0.5, 4.0, 2.0, 1.5, 0.75], rtol=1e-14)
    t8 = np.concatenate([t[:6], [0.0, 0.0]])                    # angle vector: rtx = rty = 0 keeps the anchor's angle
    np.testing.assert_allclose(D.decode(t8, a, angle_vec=True)[6], 0.5, rtol=1e-14)
    np.testing.assert_allclose(D.decode(t, a, smooth=True)[3:6], [(np.log(2.0) + 1) * 2, (np.log(0.5) + 1) * 4, 1.5], rtol=1e-14)


@pytest.mark.parametrize("name", [s[0] for s in D.gpu_scenes()])
def test_margin_condition_of_every_gpu_scene(name):
    """A condition on the scenes, not a tolerance on the kernels.  fp32 expf / sigmoid differ from float64 by a few 2^-24 relative: <= ~2e-7 on a
    score, ~2e-6 m on a coordinate <= 10 m, which moves an IoU of metre-sized boxes by 1e-6 .. 1e-5.  With every margin at least ten times
    that, the fp32 path and the float64 restatement take the same decisions, so the GPU tests compare integers exactly and leave no case out."""
    _, fr, cfg = D.by_name(name)
    m1, m2, m3 = D.margins(fr, cfg)
    print("[margins] %s: threshold %.2e, score gap %.2e, IoU %.2e" % (name, m1, m2, m3))
    assert m1 >= 1e-5 and m2 >= 1e-6 and m3 >= 1e-4


def test_scenes_exercise_the_cuts():
    fr0, fr1, fr2 = D.batch_frames()
    for rot in (True, False):
        cfg = dict(D.CFG, rotate=rot)
        r0, r1, r2 = D.predict_frame(fr0, cfg), D.predict_frame(fr1, cfg), D.predict_frame(fr2, cfg)
        assert r0["num_pass"] > cfg["pre_max"] and r0["num_det"] == cfg["post_max"]          # both caps bite
        assert D.predict_frame(fr0, dict(cfg, post_max=cfg["pre_max"]))["num_det"] > cfg["post_max"]
        assert 0 < r1["num_pass"] < 64 and 0 < r1["num_det"] < r1["num_pass"]                # one partial mask block, some suppression
        assert r2["num_pass"] == 0 and r2["num_det"] == 0


def test_struct_mirrors_have_the_library_sizes():
    lib = _lib.load()
    assert ctypes.sizeof(detect.DetPostDesc) == lib.papc_abi_sizeof(b"papc_det_post_desc") == 64
    assert ctypes.sizeof(detect.DetPostIo) == lib.papc_abi_sizeof(b"papc_det_post_io") == 12 * ctypes.sizeof(ctypes.c_void_p)


def _desc(**kw):
    base = dict(B=1, A=286, num_cls=1, score_mode=0, use_dir=1, use_rotate_nms=1, encode_angle_to_vector=0, smooth_dim=0, code_size=7, pre_max=100,
                post_max=40, score_thresh=0.15, iou_thresh=0.5, anchor_batch_stride=0)
    base.update(kw)
    return detect.DetPostDesc(**base)


BAD = ctypes.c_size_t(-1).value


@pytest.mark.parametrize("kw,word", [(dict(pre_max=4097), b"pre_max"), (dict(pre_max=0), b"pre_max"), (dict(post_max=101), b"post_max"),
                                     (dict(post_max=0), b"post_max"), (dict(num_cls=17), b"num_cls"), (dict(score_mode=3), b"score_mode"),
                                     (dict(score_mode=1, num_cls=1), b"num_cls"), (dict(code_size=8), b"code_size"),
                                     (dict(encode_angle_to_vector=1), b"code_size"), (dict(B=1 << 16, A=1 << 15), b"2^31"), (dict(A=0), b"A=0")])
def test_limits_are_refused_on_the_host(kw, word):
    lib = _lib.load()
    d = _desc(**kw)
    io = detect.DetPostIo()
    assert lib.papc_det_post_workspace(ctypes.byref(d)) == BAD            # the size_t spelling of -1
    assert word in lib.papc_last_error_string()
    assert lib.papc_det_post_f32(ctypes.byref(d), ctypes.byref(io), None, 0, None) == -1
    assert word in lib.papc_last_error_string()


def test_null_pointers_are_refused_on_the_host():
    lib = _lib.load()
    assert lib.papc_det_post_workspace(None) == BAD and b"null" in lib.papc_last_error_string()
    d = _desc()
    assert lib.papc_det_post_f32(None, None, None, 0, None) == -1 and b"null" in lib.papc_last_error_string()
    assert lib.papc_det_post_f32(ctypes.byref(d), None, None, 0, None) == -1 and b"null" in lib.papc_last_error_string()
    io = detect.DetPostIo()                                               # every pointer NULL, with a non-null workspace address
    assert lib.papc_det_post_f32(ctypes.byref(d), ctypes.byref(io), 256, 1 << 30, None) == -1 and b"null" in lib.papc_last_error_string()
    assert lib.papc_box_decode_f32(None, None, 1, 7, 0, 0, None, None) == -1 and b"null" in lib.papc_last_error_string()
    assert lib.papc_box_decode_f32(256, 256, 1, 8, 0, 0, 256, None) == -1 and b"code_size" in lib.papc_last_error_string()
    assert lib.papc_box_decode_f32(256, 256, 1, 7, 1, 0, 256, None) == -1 and b"code_size" in lib.papc_last_error_string()
    assert lib.papc_box_decode_f32(256, 256, 0, 7, 0, 0, 256, None) == -1


def test_python_layer_refuses_what_is_not_built():
    kw = dict(num_class=1, nms_score_threshold=0.15, nms_pre_max_size=100, nms_post_max_size=40, nms_iou_threshold=0.5)
    box, cls, dirp, anc = torch.zeros(1, 8, 7), torch.zeros(1, 8, 1), torch.zeros(1, 8, 2), torch.zeros(1, 8, 7)
    example = {"anchors": anc, "image_idx": [0]}
    preds = {"box_preds": box, "cls_preds": cls, "dir_cls_preds": dirp}
    with pytest.raises(_lib.PapcError, match="multiclass_nms"):
        detect.predict(example, preds, multiclass_nms=True, **kw)
    with pytest.raises(_lib.PapcError, match="no CPU fallback"):                 # CPU tensors, like nms.py
        detect.predict_tensors(box, cls, dirp, anc, fused=True, **kw)
    with pytest.raises(_lib.PapcError, match="no CPU fallback"):
        detect.predict(example, preds, fused=True, **kw)
    with pytest.raises(_lib.PapcError, match="no CPU fallback"):
        detect.second_box_decode(box, anc, fused=True)
    with pytest.raises(_lib.PapcError, match="pre_max"):
        detect.workspace_bytes(1, 286, 1, 4097, 40)


def test_switch_is_read_at_import():
    assert detect.fused_enabled() is True or detect.fused_enabled() is False
