"""A float64 / numpy restatement of the non-multiclass ``predict()`` path (pointpillars/models/detectors/pointpillars.py:218-398 with
second_box_decode, center_to_corner_box2d, corner_to_standup_nd, nms / rotate_nms of libs/ops/box_paddle_ops.py) under the project's one
order: descending score, on exactly equal scores descending anchor index, for the top-k cut and the sweep alike.  Equal class scores give
the lowest label, dir[0] == dir[1] gives direction label 0.  Suppression is ``oracle.reference_np.nms_gpu`` / ``rotate_nms_gpu`` on the
fp32 casts of the float64 boxes.  The scenes (ours, not the reference's) and the settings the GPU tests use are listed here once, so that
tests/test_detpost_host.py can hold every one of them to the margin condition that makes exact comparisons legitimate."""
import functools

import numpy as np

from oracle import reference_np as R

GRID = (13, 11)           # cells, 0.64 m pitch, two anchors per cell (r = 0, pi/2): A = 286, no multiple of 64 or 256
A = GRID[0] * GRID[1] * 2
CFG = dict(score_thresh=0.15, iou_thresh=0.5, pre_max=100, post_max=40, mode=0, use_dir=True, angle_vec=False, smooth=False)


def anchors_grid():
    ix, iy, ir = np.meshgrid(np.arange(GRID[0]), np.arange(GRID[1]), np.arange(2), indexing="ij")
    a = np.zeros((A, 7), np.float32)
    a[:, 0] = ((ix - GRID[0] // 2) * 0.64).reshape(-1)
    a[:, 1] = ((iy - GRID[1] // 2) * 0.64).reshape(-1)
    a[:, 2] = -1.78
    a[:, 3:6] = (1.6, 3.9, 1.56)
    a[:, 6] = (ir * (np.pi / 2)).reshape(-1)
    return a


def scene(seed, hot, num_cls=1, code=7):
    """one frame: encodings N(0, 0.15), cold logits -4 + N(0, 0.05), ``hot`` anchors drawn without replacement get logits U(-3, 3)"""
    rng = np.random.default_rng(seed)
    box = rng.normal(0.0, 0.15, (A, code)).astype(np.float32)
    cls = (-4.0 + rng.normal(0.0, 0.05, (A, num_cls))).astype(np.float32)
    if hot:
        idx = rng.choice(A, hot, replace=False)
        cls[idx, rng.integers(0, num_cls, hot)] = rng.uniform(-3.0, 3.0, hot).astype(np.float32)
    dirp = rng.normal(0.0, 1.0, (A, 2)).astype(np.float32)
    return dict(box=box, cls=cls, dir=dirp, anchors=anchors_grid(), mask=None)


def third_mask(seed):
    return (np.random.default_rng(1000 + seed).uniform(size=A) < 1.0 / 3.0).astype(np.uint8)


# (name, frame, settings): every random frame a GPU test runs, with the settings it runs under.  Frames with engineered exact ties are built in
# the GPU test itself: the margin condition is about near-ties, and those frames have none by construction of their few distinct values.
SEED_HOT150, SEED_HOT40, SEED_COLD, SEED_MASKED = 4, 12, 3, 5


def batch_frames():
    return [scene(SEED_HOT150, 150), scene(SEED_HOT40, 40), scene(SEED_COLD, 0)]


def gpu_scenes():
    out = []
    for rot in (True, False):
        for i, fr in enumerate(batch_frames()):
            out.append(("batch%d_rot%d" % (i, rot), fr, dict(CFG, rotate=rot)))
    masked = dict(scene(SEED_MASKED, 150), mask=third_mask(SEED_MASKED))
    out.append(("masked_thresh0", masked, dict(CFG, rotate=True, score_thresh=0.0)))
    for K, P in ((64, 40), (65, 40), (100, 1), (4096, 40)):
        out.append(("cap_K%d_P%d" % (K, P), scene(SEED_HOT150, 150), dict(CFG, rotate=True, pre_max=K, post_max=P)))
    out.append(("mode1_c4", scene(2, 150, num_cls=4), dict(CFG, rotate=True, mode=1)))
    out.append(("mode2_c4", scene(2, 150, num_cls=4), dict(CFG, rotate=True, mode=2, score_thresh=0.5)))
    out.append(("mode0_c3", scene(2, 150, num_cls=3), dict(CFG, rotate=False, mode=0)))
    out.append(("reuse_small", scene(16, 40), dict(CFG, rotate=True)))
    return out


def decode(t, a, angle_vec=False, smooth=False):
    """second_box_decode (box_paddle_ops.py:48-83) in float64"""
    t, a = np.asarray(t, np.float64), np.asarray(a, np.float64)
    xa, ya, za, wa, la, ha, ra = [a[..., i] for i in range(7)]
    za = za + ha / 2
    diagonal = np.sqrt(la ** 2 + wa ** 2)
    xg, yg, zg = t[..., 0] * diagonal + xa, t[..., 1] * diagonal + ya, t[..., 2] * ha + za
    if smooth:
        lg, wg, hg = (t[..., 4] + 1) * la, (t[..., 3] + 1) * wa, (t[..., 5] + 1) * ha
    else:
        lg, wg, hg = np.exp(t[..., 4]) * la, np.exp(t[..., 3]) * wa, np.exp(t[..., 5]) * ha
    rg = np.arctan2(t[..., 7] + np.sin(ra), t[..., 6] + np.cos(ra)) if angle_vec else t[..., 6] + ra
    zg = zg - hg / 2
    return np.stack([xg, yg, zg, wg, lg, hg, rg], -1)


def scores_of(cls, mode):
    cls = np.asarray(cls, np.float64)
    if mode == 2:
        e = np.exp(cls - cls.max(-1, keepdims=True))
        total = (e / e.sum(-1, keepdims=True))[..., 1:]
    else:
        total = 1.0 / (1.0 + np.exp(-cls))
        if mode == 1:
            total = total[..., 1:]
    return total.max(-1), total.argmax(-1)            # numpy's argmax returns the first maximum: the lowest class


def nms_boxes(box, rotate):
    nb = box[:, [0, 1, 3, 4, 6]]
    if rotate:
        return nb
    corners = R.center_to_corner_box2d(nb[:, :2], nb[:, 2:4], nb[:, 4])
    return R.corner_to_standup_nd(corners)


def candidates(fr, cfg):
    """everything up to the NMS call: (num_pass, rank-ordered anchor indices of the first K, their boxes / NMS boxes / scores / labels / dir labels)"""
    top, lab = scores_of(fr["cls"], cfg["mode"])
    ok = np.ones(top.shape[0], bool) if fr["mask"] is None else fr["mask"] != 0
    if cfg["score_thresh"] > 0:
        ok &= top >= np.float64(np.float32(cfg["score_thresh"]))
    idx = np.nonzero(ok)[0]
    order = idx[np.argsort(top[idx], kind="stable")[::-1]][:cfg["pre_max"]]
    box = decode(fr["box"][order], fr["anchors"][order], cfg["angle_vec"], cfg["smooth"])
    dl = (fr["dir"][order, 1] > fr["dir"][order, 0]).astype(np.int64) if cfg["use_dir"] else np.zeros(order.shape[0], np.int64)
    return int(idx.shape[0]), order, box, nms_boxes(box, cfg["rotate"]), top[order], lab[order], dl


def predict_frame(fr, cfg):
    """-> dict(num_pass, num_det, anchor_idx, labels, dir_labels, scores, boxes) of one frame, unpadded"""
    n_pass, order, box, nb, sc, lab, dl = candidates(fr, cfg)
    if order.shape[0] == 0:
        keep = np.zeros(0, np.int64)
    else:
        # the oracle sorts once more (descending score, higher row first on equal scores): rows handed over in reverse rank order come back in rank order
        dets = np.concatenate([nb, sc[:, None]], 1).astype(np.float32)[::-1]
        sel = (R.rotate_nms_gpu if cfg["rotate"] else R.nms_gpu)(dets, cfg["iou_thresh"])
        keep = (dets.shape[0] - 1 - np.asarray(sel, np.int64))[:cfg["post_max"]]
    box = box[keep].copy()
    if cfg["use_dir"]:
        box[:, 6] += np.where((box[:, 6] > 0) ^ (dl[keep] != 0), np.float64(np.float32(np.pi)), 0.0)
    return dict(num_pass=n_pass, num_det=int(keep.shape[0]), anchor_idx=order[keep], labels=lab[keep], dir_labels=dl[keep], scores=sc[keep], boxes=box)


def margins(fr, cfg):
    """(i) the smallest |score - score_thresh| over unmasked anchors, (ii) the smallest gap between consecutive distinct scores among passing
    anchors, (iii) the smallest |IoU - iou_thresh| over the pairs among the first K.  inf where there is nothing to compare."""
    top, _ = scores_of(fr["cls"], cfg["mode"])
    un = np.ones(top.shape[0], bool) if fr["mask"] is None else fr["mask"] != 0
    m1 = float(np.min(np.abs(top[un] - cfg["score_thresh"]))) if cfg["score_thresh"] > 0 and un.any() else np.inf
    ok = un & (top >= cfg["score_thresh"]) if cfg["score_thresh"] > 0 else un
    gaps = np.diff(np.unique(top[ok]))
    m2 = float(gaps.min()) if gaps.size else np.inf
    _, order, _, nb, sc, _, _ = candidates(fr, cfg)
    m3 = np.inf
    n = order.shape[0]
    if n >= 2:
        if cfg["rotate"]:
            dets = np.concatenate([nb, sc[:, None]], 1).astype(np.float32)[::-1]
            _, ious = R.rotate_nms_gpu(dets, cfg["iou_thresh"], return_ious=True)
            v = np.asarray(list(ious.values()), np.float64)
        else:
            b = nb.astype(np.float32)
            v = np.asarray([R.nms_iou(b[i], b[j]) for i in range(n) for j in range(i + 1, n)], np.float64)
        m3 = float(np.min(np.abs(v - np.float64(np.float32(cfg["iou_thresh"])))))
    return m1, m2, m3


@functools.lru_cache(maxsize=None)
def _cached(i):
    name, fr, cfg = gpu_scenes()[i]
    return predict_frame(fr, cfg)


def expected(name):
    """the restatement's result for a named scene of gpu_scenes(), computed once per process"""
    names = [s[0] for s in gpu_scenes()]
    return _cached(names.index(name))


def by_name(name):
    for s in gpu_scenes():
        if s[0] == name:
            return s
    raise KeyError(name)
