"""GPU parity of the predict() stage (papc_amd.detect on csrc/detpost.hip) with the float64 restatement tests/detpost_ref.py.  Integer outputs
are compared exactly: tests/test_detpost_host.py holds every random scene used here to the margin condition that makes that legitimate."""
import numpy as np
import pytest
import torch

from tests import detpost_ref as D
from tests.util import assert_close

pytestmark = pytest.mark.gpu

INT_KEYS = ("labels", "dir_labels", "anchor_idx")


def _kw(cfg, num_cls):
    return dict(num_class=num_cls if cfg["mode"] == 0 else num_cls - 1, encode_background_as_zeros=cfg["mode"] == 0,
                use_sigmoid_score=cfg["mode"] != 2, use_direction_classifier=cfg["use_dir"], use_rotate_nms=cfg["rotate"],
                nms_score_threshold=cfg["score_thresh"], nms_pre_max_size=cfg["pre_max"], nms_post_max_size=cfg["post_max"],
                nms_iou_threshold=cfg["iou_thresh"], encode_angle_to_vector=cfg["angle_vec"], smooth_dim=cfg["smooth"])


def _poisoned(B, P):
    """output buffers pre-filled with NaN / a sentinel: every element must be written"""
    dev = "cuda"
    return {"boxes": torch.full((B, P, 7), float("nan"), device=dev), "scores": torch.full((B, P), float("nan"), device=dev),
            "labels": torch.full((B, P), -77, dtype=torch.int32, device=dev), "dir_labels": torch.full((B, P), -77, dtype=torch.int32, device=dev),
            "anchor_idx": torch.full((B, P), -77, dtype=torch.int32, device=dev), "num_det": torch.full((B,), -77, dtype=torch.int32, device=dev),
            "num_pass": torch.full((B,), -77, dtype=torch.int32, device=dev)}


def _run(frames, cfg, shared_anchors=False, fused=True, workspace=None):
    from papc_amd import detect
    t = lambda k: torch.from_numpy(np.stack([f[k] for f in frames])).cuda()      # noqa: E731
    anchors = torch.from_numpy(frames[0]["anchors"]).cuda() if shared_anchors else t("anchors")
    mask = None if frames[0]["mask"] is None else t("mask")
    out = _poisoned(len(frames), cfg["post_max"])
    r = detect.predict_tensors(t("box"), t("cls"), t("dir"), anchors, mask, fused=fused, workspace=workspace, out=out,
                               **_kw(cfg, frames[0]["cls"].shape[-1]))
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check_frame(got, b, want, P, what):
    n = want["num_det"]
    assert got["num_pass"][b] == want["num_pass"], (what, got["num_pass"][b], want["num_pass"])
    assert got["num_det"][b] == n, (what, got["num_det"][b], n)
    for k in INT_KEYS:
        assert got[k][b, :n].tolist() == want[k].tolist(), (what, k)
    if n:
        assert_close(got["scores"][b, :n], want["scores"], rel=1e-6, what=what + " scores")
        assert_close(got["boxes"][b, :n], want["boxes"], rel=1e-6, what=what + " boxes")       # column 6 after the direction flip
    assert (got["boxes"][b, n:] == 0).all() and (got["scores"][b, n:] == 0).all()              # padding: exactly 0 / -1, no NaN left
    assert (got["labels"][b, n:] == 0).all() and (got["dir_labels"][b, n:] == 0).all() and (got["anchor_idx"][b, n:] == -1).all()


def _same_bits(x, y):
    return all(np.array_equal(x[k].view(np.int32) if x[k].dtype == np.float32 else x[k], y[k].view(np.int32) if y[k].dtype == np.float32 else y[k])
               for k in x)


@pytest.mark.parametrize("angle_vec", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("n", [1, D.A * 3])
def test_second_box_decode_against_float64(n, smooth, angle_vec):
    from papc_amd import detect
    rng = np.random.default_rng(100 + n + 2 * smooth + angle_vec)
    enc = rng.normal(0.0, 0.15, (n, 8 if angle_vec else 7)).astype(np.float32)
    anc = np.tile(D.anchors_grid(), (3, 1))[:n]
    got = detect.second_box_decode(torch.from_numpy(enc).cuda(), torch.from_numpy(anc).cuda(), angle_vec, smooth, fused=True).cpu().numpy()
    ref = D.decode(enc, anc, angle_vec, smooth)
    assert_close(got, ref, rel=1e-6, what="second_box_decode n=%d smooth=%d angle_vec=%d" % (n, smooth, angle_vec))
    # every element within 1e-6 of the magnitude of ITS OWN terms: x = xt d + xa is a sum that may cancel (a centre near 0 from terms of metres), and
    # fp32 rounds the terms, so the terms' size -- not the sum's -- is what a handful of fp32 operations can be held to
    t, an = enc.astype(np.float64), anc.astype(np.float64)
    diag = np.sqrt(an[:, 4] ** 2 + an[:, 3] ** 2)
    scale = np.abs(ref)
    scale[:, 0] = np.abs(t[:, 0]) * diag + np.abs(an[:, 0])
    scale[:, 1] = np.abs(t[:, 1]) * diag + np.abs(an[:, 1])
    scale[:, 2] = np.abs(t[:, 2] * an[:, 5]) + np.abs(an[:, 2]) + an[:, 5] / 2 + ref[:, 5] / 2
    scale[:, 6] = 1.0 + np.abs(ref[:, 6]) if angle_vec else np.abs(t[:, 6]) + np.abs(an[:, 6])      # atan2 of O(1) sums / rt + ra
    worst = float(np.max(np.abs(got - ref) / np.maximum(scale, 1e-30)))
    print("[decode] elementwise error over the size of the element's terms: %.2e (bar 1e-6)" % worst)
    assert worst <= 1e-6


@pytest.mark.parametrize("rot", [True, False])
def test_three_frame_batch(rot):
    """frame 0 passes more than K anchors and keeps more than P, frame 1 passes fewer than 64 (one partial mask block), frame 2 none"""
    cfg = dict(D.CFG, rotate=rot)
    got = _run(D.batch_frames(), cfg)
    for b in range(3):
        _check_frame(got, b, D.expected("batch%d_rot%d" % (b, rot)), cfg["post_max"], "frame %d rot=%d" % (b, rot))
    assert got["num_det"].tolist() == [cfg["post_max"], D.expected("batch1_rot%d" % rot)["num_det"], 0] and got["num_pass"][0] > cfg["pre_max"]


def _tie_frame():
    """32 disjoint anchors 20 m apart, two class columns.  Four anchors with distinct scores in column 1, eight that share ONE logit bit for
    bit in BOTH columns (equal class scores) with identical encodings and dir[0] == dir[1], the rest cold."""
    n = 32
    anchors = np.tile(np.array([[0, 0, -1.78, 1.6, 3.9, 1.56, 0.0]], np.float32), (n, 1))
    anchors[:, 0] = 20.0 * np.arange(n)
    box = np.tile(np.random.default_rng(5).normal(0.0, 0.15, (1, 7)).astype(np.float32), (n, 1))
    cls = np.full((n, 2), -4.0, np.float32)
    dirp = np.tile(np.array([[0.0, 1.0]], np.float32), (n, 1))
    for i, v in zip((1, 10, 18, 25), (2.0, 1.5, 1.0, 0.75)):
        cls[i, 1] = v
    tied = [3, 7, 9, 12, 15, 20, 21, 30]
    cls[tied] = np.float32(0.5)
    dirp[tied] = np.float32(0.3)
    return dict(box=box, cls=cls, dir=dirp, anchors=anchors, mask=None), tied


@pytest.mark.parametrize("rot", [True, False])
def test_engineered_exact_ties(rot):
    """K = 9 cuts through the eight tied anchors: after the four distinct ones the tie rule takes the highest anchor indices first.  Equal class
    logits give label 0 (the distinct anchors score in column 1: label 1), dir[0] == dir[1] gives dir label 0."""
    fr, tied = _tie_frame()
    cfg = dict(D.CFG, rotate=rot, pre_max=9, post_max=9)
    got = _run([fr], cfg)
    assert got["num_pass"][0] == 12 and got["num_det"][0] == 9
    assert got["anchor_idx"][0].tolist() == [1, 10, 18, 25] + sorted(tied, reverse=True)[:5]
    assert got["labels"][0].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert got["dir_labels"][0].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert len(set(got["scores"][0, 4:].view(np.int32).tolist())) == 1                         # one score, bit for bit
    _check_frame(got, 0, D.predict_frame(fr, cfg), 9, "ties rot=%d" % rot)
    got = _run([fr], dict(cfg, post_max=6))                                                    # P cuts through them as well
    assert got["anchor_idx"][0].tolist() == [1, 10, 18, 25, 30, 21]


@pytest.mark.parametrize("name", ["mode1_c4", "mode2_c4", "mode0_c3"])
def test_score_modes_and_class_count(name):
    _, fr, cfg = D.by_name(name)
    got = _run([fr], cfg)
    want = D.expected(name)
    _check_frame(got, 0, want, cfg["post_max"], name)
    assert len(set(want["labels"].tolist())) > 1                                               # more than one label is exercised


def test_threshold_zero_with_anchor_mask():
    """score_thresh = 0: every unmasked anchor passes; masked anchors never appear and the indices count in the unmasked numbering"""
    name, fr, cfg = D.by_name("masked_thresh0")
    got = _run([fr], cfg)
    assert got["num_pass"][0] == int(fr["mask"].sum())
    n = got["num_det"][0]
    assert (fr["mask"][got["anchor_idx"][0, :n]] != 0).all()
    _check_frame(got, 0, D.expected(name), cfg["post_max"], name)


@pytest.mark.parametrize("K,P", [(64, 40), (65, 40), (100, 1), (4096, 40)])
def test_caps(K, P):
    name, fr, cfg = D.by_name("cap_K%d_P%d" % (K, P))
    got = _run([fr], cfg)
    _check_frame(got, 0, D.expected(name), P, name)


def test_shared_anchor_set_equals_the_tiled_one():
    cfg = dict(D.CFG, rotate=True)
    assert _same_bits(_run(D.batch_frames(), cfg, shared_anchors=True), _run(D.batch_frames(), cfg))


def test_workspace_reuse_and_determinism():
    """a larger batch first, then a smaller frame on the SAME workspace: no stale count, key or mask word leaks; and the same input twice gives the same bits"""
    from papc_amd import detect
    cfg = dict(D.CFG, rotate=True)
    _, small, _ = D.by_name("reuse_small")
    ws = torch.empty(detect.workspace_bytes(3, D.A, 1, cfg["pre_max"], cfg["post_max"]), dtype=torch.uint8, device="cuda")
    big1 = _run(D.batch_frames(), cfg, workspace=ws)
    reused = _run([small], cfg, workspace=ws)
    fresh = _run([small], cfg)
    assert _same_bits(reused, fresh)
    _check_frame(reused, 0, D.expected("reuse_small"), cfg["post_max"], "reuse_small")
    assert _same_bits(big1, _run(D.batch_frames(), cfg, workspace=ws))


@pytest.mark.parametrize("rot", [True, False])
def test_fused_and_torch_op_legs_agree(rot):
    cfg = dict(D.CFG, rotate=rot)
    a, b = _run(D.batch_frames(), cfg, fused=True), _run(D.batch_frames(), cfg, fused=False)
    for k in INT_KEYS + ("num_det", "num_pass"):
        assert np.array_equal(a[k], b[k]), k
    assert_close(a["scores"], b["scores"], rel=1e-6, what="legs scores rot=%d" % rot)
    assert_close(a["boxes"], b["boxes"], rel=1e-6, what="legs boxes rot=%d" % rot)


def _dense_frame(N, rot):
    """N anchors on a jittered 13-column grid, pitched so that neighbours overlap past the threshold and second neighbours do not (the axis-aligned
    IoU counts a "+1" per side, hence its wider pitch); zero encodings, so a decoded box is its anchor's floats exactly (0 * d + xa, expf(0) * wa,
    0 + ra); one class column of N distinct logits in [-2, 2], at least 0.03 apart, shuffled: sigmoid gaps of 3e-3 and more, which no two
    roundings of a sigmoid reorder.  Seed 33: no pair's IoU within 8e-4 of the threshold, 18 to 51 boxes suppressed in the four cases."""
    rng = np.random.default_rng(33)
    px, py, jit = (0.45, 1.2, 0.15) if rot else (0.8, 2.0, 0.3)
    i = np.arange(N)
    anchors = np.zeros((N, 7), np.float32)
    anchors[:, 0] = (i % 13) * px + rng.uniform(-jit, jit, N)
    anchors[:, 1] = (i // 13) * py + rng.uniform(-jit, jit, N)
    anchors[:, 2] = -1.78
    anchors[:, 3:6] = (1.6, 3.9, 1.56)
    anchors[:, 6] = rng.uniform(-0.6, 0.6, N) if rot else 0.0
    cls = rng.permutation(np.linspace(-2.0, 2.0, N)).astype(np.float32)[:, None]
    return dict(box=np.zeros((N, 7), np.float32), cls=cls, dir=np.zeros((N, 2), np.float32), anchors=anchors, mask=None)


@pytest.mark.parametrize("N", [65, 130])
@pytest.mark.parametrize("rot", [True, False])
def test_suppression_agrees_with_the_standalone_nms(rot, N):
    """predict()'s suppression and nms.rotate_nms_gpu_tensor / nms.nms_gpu_tensor run one tile and one sweep (csrc/nms_iou.h): on the same boxes
    and scores they keep the same anchors in the same order.  N = 65 and 130: two and three column blocks, a partial last one, off-diagonal
    tiles on both sides of a block edge.  With r = 0 the stand-up box is exactly (x - w/2, y - l/2, x + w/2, y + l/2): cos 0 = 1 and
    sin 0 = 0 leave each corner term exact."""
    from papc_amd import detect, nms
    fr = _dense_frame(N, rot)
    cfg = dict(D.CFG, rotate=rot, score_thresh=0.0, pre_max=N, post_max=N, use_dir=False)
    cls = torch.from_numpy(fr["cls"][None]).cuda()
    anchors = torch.from_numpy(fr["anchors"]).cuda()
    r = detect.predict_tensors(torch.from_numpy(fr["box"][None]).cuda(), cls, None, anchors, None, fused=True, **_kw(cfg, 1))
    n = int(r["num_det"][0])
    x, y, w, l, ang = (anchors[:, k] for k in (0, 1, 3, 4, 6))
    score = torch.sigmoid(cls[0, :, 0])
    if rot:
        keep = nms.rotate_nms_gpu_tensor(torch.stack([x, y, w, l, ang, score], dim=1), cfg["iou_thresh"])
    else:
        keep = nms.nms_gpu_tensor(torch.stack([x - w / 2, y - l / 2, x + w / 2, y + l / 2, score], dim=1), cfg["iou_thresh"])
    print("[nms agreement] rot=%d N=%d kept %d suppressed %d" % (rot, N, n, N - n))
    assert n >= N / 8 and N - n >= N / 8                                                       # neither side of the decision is vacuous
    assert int(r["num_pass"][0]) == N
    assert r["anchor_idx"][0, :n].tolist() == keep.tolist()


def test_predict_dict_interface_on_rpn_maps():
    """predict() on the RPN's [B,H,W,.] maps: the source's list of dicts, None entries for the frame without a detection"""
    from papc_amd import detect
    frames = D.batch_frames()
    cfg = dict(D.CFG, rotate=True)
    H, W = D.GRID
    t = lambda k, c: torch.from_numpy(np.stack([f[k] for f in frames])).cuda().reshape(3, H, W, 2 * c)      # noqa: E731
    example = {"anchors": torch.from_numpy(np.stack([f["anchors"] for f in frames])).cuda().reshape(3, H, W, 2, 7), "image_idx": [7, 8, 9]}
    preds = {"box_preds": t("box", 7), "cls_preds": t("cls", 1), "dir_cls_preds": t("dir", 2)}
    out = detect.predict(example, preds, fused=True, **_kw(cfg, 1))
    assert [o["image_idx"] for o in out] == [7, 8, 9]
    for b in range(2):
        want = D.expected("batch%d_rot1" % b)
        assert set(out[b]) == {"bbox", "box3d_camera", "box3d_lidar", "scores", "label_preds", "image_idx"}
        assert out[b]["bbox"] is None and out[b]["box3d_camera"] is None
        assert out[b]["label_preds"].dtype == torch.int64 and out[b]["label_preds"].tolist() == want["labels"].tolist()
        assert tuple(out[b]["box3d_lidar"].shape) == (want["num_det"], 7)
        assert_close(out[b]["box3d_lidar"].cpu().numpy(), want["boxes"], rel=1e-6, what="predict() frame %d boxes" % b)
        assert_close(out[b]["scores"].cpu().numpy(), want["scores"], rel=1e-6, what="predict() frame %d scores" % b)
    assert out[2]["box3d_lidar"] is None and out[2]["scores"] is None and out[2]["label_preds"] is None and out[2]["image_idx"] == 9
