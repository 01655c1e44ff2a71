"""The scenes of tests/golden/ref_dettarget.npz: generator settings and the inputs (pillar coordinates, padded ground-truth batches) that
tests/golden/make_dettarget_golden.py feeds to the reference's own functions.  The recorder stores the inputs next to the recorded outputs,
so the tests read every array from the file and take from here only the settings: the generators' constructor arguments, the grid geometry,
the switches and the names.  The second half holds what the host and the GPU tests share: the loader, the cache builder, the comparison."""
import functools
import os

import numpy as np

CAR = dict(sizes=[1.6, 3.9, 1.56], rotations=[0, np.pi / 2], match_threshold=0.6, unmatch_threshold=0.45)
NAN_ROW = np.float32("nan")


def _geometry(H, W, voxel, y0):
    """pillar grid 2W x 2H cells of ``voxel`` metres from (0, y0); feature map H x W at twice that stride"""
    nx, ny = 2 * W, 2 * H
    return dict(fmap=(1, H, W), voxel_size=np.array([voxel, voxel, 4.0], np.float32),
                pc_range=np.array([0.0, y0, -3.0, nx * voxel, y0 + ny * voxel, 1.0], np.float32), grid_size=(nx, ny, 1))


def _car_gen(voxel, y0, **over):
    kw = dict(CAR, anchor_strides=[2 * voxel, 2 * voxel, 0.0], anchor_offsets=[voxel, y0 + voxel, -1.78])
    kw.update(over)
    return ("stride", kw)


def _pillars(rng, b, nx, ny, x_cells, frac):
    """a random ``frac`` of the cells with x < x_cells, as coors rows (batch, z, y, x)"""
    ys, xs = np.nonzero(rng.random((ny, x_cells)) < frac)
    return np.stack([np.full_like(ys, b), np.zeros_like(ys), ys, xs], axis=1).astype(np.int32)


def _gts(rng, n, x_hi, y_lo, y_hi):
    g = np.empty((n, 7), np.float32)
    g[:, 0] = rng.uniform(1.0, x_hi, n)
    g[:, 1] = rng.uniform(y_lo, y_hi, n)
    g[:, 2] = rng.uniform(-1.9, -1.6, n)
    g[:, 3] = rng.uniform(1.4, 1.8, n)
    g[:, 4] = rng.uniform(3.5, 4.3, n)
    g[:, 5] = rng.uniform(1.4, 1.7, n)
    g[:, 6] = np.where(rng.random(n) < 0.5, rng.uniform(-0.2, 0.2, n) + rng.integers(0, 2, n) * (np.pi / 2), rng.uniform(-np.pi, np.pi, n))
    return g


def _batch(frames, gmax):
    """frames: a list of (gt [n,7], classes [n]) -> gt_boxes [B,gmax,7] / gt_classes [B,gmax] / num_gt [B]; the rows past n hold NaN and -99"""
    B = len(frames)
    boxes = np.full((B, gmax, 7), NAN_ROW, np.float32)
    classes = np.full((B, gmax), -99, np.int32)
    for b, (g, c) in enumerate(frames):
        boxes[b, :len(g)], classes[b, :len(g)] = g, c
    return dict(gt_boxes=boxes, gt_classes=classes, num_gt=np.array([len(g) for g, _ in frames], np.int32))


def scene_a(angle_vec=False, smooth=False):
    rng = np.random.default_rng(2024)
    s = _geometry(21, 19, 0.4, -8.4)
    g = _gts(rng, 5, 10.0, -6.0, 6.0)
    s.update(gens=[_car_gen(0.4, -8.4)], coors=_pillars(rng, 0, 38, 42, 25, 0.3), area_thr=1, angle_vec=angle_vec, smooth=smooth,
             **_batch([(g, np.ones(5, np.int32))], 5))
    return s


def scene_b():
    """dyadic: every coordinate a multiple of 0.125, so symmetric anchors tie bit for bit"""
    s = _geometry(24, 24, 0.125, 0.0)
    gen = ("stride", dict(sizes=[1.5, 4.0, 1.5], anchor_strides=[0.25, 0.25, 0.0], anchor_offsets=[0.125, 0.125, -1.0], rotations=[0, np.pi / 2],
                          match_threshold=0.6, unmatch_threshold=0.45))
    ys, xs = np.mgrid[0:48, 0:24]                                        # every cell left of x = 3 m holds a pillar, none right of it
    coors = np.stack([np.zeros(ys.size, np.int64), np.zeros(ys.size, np.int64), ys.ravel(), xs.ravel()], axis=1).astype(np.int32)
    g = np.array([[1.5, 3.125, -1.0, 1.5, 4.0, 1.5, 0.0],                # midway between the anchor centres x = 1.375 and x = 1.625
                  [2.125, 1.125, -1.0, 1.5, 4.0, 1.5, 0.0],              # exactly on an anchor
                  [100.0, 100.0, -1.0, 1.5, 4.0, 1.5, 0.0],              # overlaps nothing
                  [1.0, 4.5, -1.0, 0.5, 0.5, 1.5, 0.0],                  # class 2, small: every anchor that contains it ties at 0.25 / 6
                  [5.125, 3.125, -1.0, 1.5, 4.0, 1.5, 0.0]], np.float32)  # class 2, exactly on an anchor that the mask leaves out
    s.update(gens=[gen], coors=coors, area_thr=1, angle_vec=False, smooth=False, **_batch([(g, np.array([1, 1, 1, 2, 2], np.int32))], 5))
    return s


def scene_c():
    rng = np.random.default_rng(77)
    s = _geometry(21, 19, 0.4, -8.4)
    coors = np.concatenate([_pillars(rng, 0, 38, 42, 30, 0.3), _pillars(rng, 1, 38, 42, 20, 0.4)])      # frame 2 has no pillar: its mask is all zero
    g0, g2 = _gts(rng, 33, 11.0, -7.0, 7.0), _gts(rng, 1, 8.0, -4.0, 4.0)
    frames = [(g0, rng.integers(1, 3, 33).astype(np.int32)), (g0[:0], np.zeros(0, np.int32)), (g2, np.ones(1, np.int32))]
    s.update(gens=[_car_gen(0.4, -8.4)], coors=coors, area_thr=1, angle_vec=False, smooth=False, **_batch(frames, 33))
    return s


def scene_d():
    rng = np.random.default_rng(5)
    s = _geometry(50, 44, 0.4, -20.0)
    g = _gts(rng, 6, 30.0, -16.0, 16.0)
    s.update(gens=[_car_gen(0.4, -20.0)], coors=_pillars(rng, 0, 88, 100, 80, 0.3), area_thr=1, angle_vec=False, smooth=False,
             **_batch([(g, np.ones(6, np.int32))], 6))
    return s


def scene_e():
    rng = np.random.default_rng(31)
    s = _geometry(10, 9, 0.4, -4.0)
    ped = ("range", dict(anchor_ranges=[0.4, -3.6, -0.6, 6.8, 3.6, -0.6], sizes=[0.6, 0.8, 1.73], rotations=[0, np.pi / 2], match_threshold=0.5,
                         unmatch_threshold=0.35))
    g = _gts(rng, 6, 6.0, -3.0, 3.0)
    g[3:, 3], g[3:, 4], g[3:, 5] = rng.uniform(0.5, 0.7, 3), rng.uniform(0.7, 0.9, 3), rng.uniform(1.6, 1.8, 3)
    s.update(gens=[_car_gen(0.4, -4.0), ped], coors=_pillars(rng, 0, 18, 20, 18, 0.4), area_thr=1, angle_vec=False, smooth=False,
             **_batch([(g, np.array([1, 1, 1, 2, 2, 2], np.int32))], 6))
    return s


def scene_g(area_thr):
    """mask only: two frames, duplicate rows, padding rows with batch -1 in between"""
    rng = np.random.default_rng(9)
    s = _geometry(21, 19, 0.4, -8.4)
    c0, c1 = _pillars(rng, 0, 38, 42, 38, 0.02), _pillars(rng, 1, 38, 42, 38, 0.01)
    pad = np.full((7, 4), -1, np.int32)
    coors = np.concatenate([c0, pad[:3], c0[::3], c1, pad[3:], c1[::2], c1[::2]])      # every third row of frame 0 twice, every second of frame 1 three times
    g = np.zeros((0, 7), np.float32)
    s.update(gens=[_car_gen(0.4, -8.4)], coors=coors, area_thr=area_thr, angle_vec=False, smooth=False,
             **_batch([(g, np.zeros(0, np.int32))] * 2, 0))
    return s


SCENES = {"a": scene_a, "b": scene_b, "c": scene_c, "d": scene_d, "e": scene_e,
          "f01": lambda: scene_a(False, True), "f10": lambda: scene_a(True, False), "f11": lambda: scene_a(True, True),
          "g0": lambda: scene_g(0), "g1": lambda: scene_g(1)}
INPUT_KEYS = ("coors", "gt_boxes", "gt_classes", "num_gt")
OUTPUT_KEYS = ("anchors", "matched_thresholds", "unmatched_thresholds", "anchors_bv", "cells", "area", "mask", "labels", "reg_targets", "reg_weights",
               "gt_ids", "max_overlap", "num_pos")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# shared by tests/test_dettarget_host.py and tests/test_gpu_dettarget.py

@functools.lru_cache(maxsize=None)
def _file():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dettarget.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def golden(name):
    """(settings, arrays) of a scene: arrays are the recorded inputs and outputs, read-only"""
    s = {k: v for k, v in SCENES[name]().items() if k not in INPUT_KEYS}
    arrays = {k: _file()["%s.%s" % (name, k)] for k in INPUT_KEYS + OUTPUT_KEYS}
    for a in arrays.values():
        a.setflags(write=False)
    return s, arrays


def make_assigner(T, s, **kw):
    gens = [(T.AnchorGeneratorStride if kind == "stride" else T.AnchorGeneratorRange)(**g) for kind, g in s["gens"]]
    return T.TargetAssigner(gens, encode_angle_to_vector=s["angle_vec"], smooth_dim=s["smooth"], **kw)


def make_cache(T, s, device):
    return T.anchor_cache(make_assigner(T, s), s["fmap"], s["voxel_size"], s["pc_range"], s["grid_size"], device=device)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def reg_target_ratio(got, g, s):
    """worst |got - golden| over the magnitude of the element's OWN terms, golden promoted to float64 (the bar is 1e-6: at most six fp32
    roundings and one logf, 6 * 2^-24 = 3.6e-7); rows without a positive label must be exactly zero"""
    ref = g["reg_targets"].astype(np.float64)
    pos = g["labels"] > 0
    assert (got[~pos] == 0).all(), "reg_targets of a row without a positive label"
    worst = 0.0
    an = g["anchors"].reshape(-1, 7).astype(np.float64)
    for b in range(ref.shape[0]):
        rows = np.nonzero(pos[b])[0]
        if rows.size == 0:
            continue
        a, gt = an[rows], g["gt_boxes"][b].astype(np.float64)[g["gt_ids"][b, rows]]
        diag = np.sqrt(a[:, 4] ** 2 + a[:, 3] ** 2)
        scale = np.maximum(1.0, np.abs(ref[b, rows]))                    # the three size columns: max(1, |log|)
        scale[:, 0] = (np.abs(gt[:, 0]) + np.abs(a[:, 0])) / diag
        scale[:, 1] = (np.abs(gt[:, 1]) + np.abs(a[:, 1])) / diag
        scale[:, 2] = (np.abs(gt[:, 2]) + gt[:, 5] / 2 + np.abs(a[:, 2]) + a[:, 5] / 2) / a[:, 5]
        if s["angle_vec"]:
            scale[:, 6:] = 2.0
        else:
            scale[:, 6] = np.abs(gt[:, 6]) + np.abs(a[:, 6])
        worst = max(worst, float(np.max(np.abs(got[b, rows].astype(np.float64) - ref[b, rows]) / np.maximum(scale, 1e-30))))
    return worst


def check_assign(got, g, s, what):
    """labels, gt_ids, num_pos, reg_weights exact; max_overlap bit for bit; reg_targets within the bar"""
    for k in ("labels", "gt_ids", "num_pos"):
        assert np.array_equal(got[k], g[k]), (what, k)
    assert np.array_equal(bits(got["max_overlap"]), bits(g["max_overlap"])), (what, "max_overlap")
    assert np.array_equal(got["reg_weights"], g["reg_weights"]), (what, "reg_weights")
    worst = reg_target_ratio(got["reg_targets"], g, s)
    print("[%s] reg_targets: worst error over the size of the element's terms %.2e (bar 1e-6)" % (what, worst))
    assert worst <= 1e-6, (what, worst)
