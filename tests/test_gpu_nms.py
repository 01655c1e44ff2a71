"""GPU parity: papc_nms_f32 vs the oracle restatement of nms_gpu (bit-exact index lists)."""
import numpy as np
import pytest
import torch

from oracle import reference_np as R
from tests import detect_cases as D

pytestmark = pytest.mark.gpu


def _boxes(rng, n, extent=200.0, size=40.0, ties=False):
    xy = rng.uniform(0, extent, (n, 2)).astype(np.float32)
    wh = rng.uniform(1, size, (n, 2)).astype(np.float32)
    sc = rng.uniform(0, 1, (n, 1)).astype(np.float32)
    if ties:
        sc = np.round(sc * 8) / np.float32(8)
    return np.concatenate([xy, xy + wh, sc], 1).astype(np.float32)


@pytest.mark.parametrize("n,thr", [(1, 0.5), (2, 0.5), (63, 0.3), (64, 0.5), (65, 0.5), (200, 0.1), (300, 0.7)])
def test_nms_matches_literal_oracle(n, thr):
    from papc_amd.nms import nms_gpu
    rng = np.random.default_rng(n)
    dets = _boxes(rng, n, extent=80.0)
    want = [int(i) for i in R.nms_gpu(dets, thr)]
    got = nms_gpu(dets, thr)
    assert got == want


@pytest.mark.parametrize("n,thr,ties", [(1000, 0.5, False), (4097, 0.3, True), (20000, 0.5, False)])
def test_nms_large_matches_vectorised_oracle(n, thr, ties):
    from papc_amd.nms import nms_gpu_tensor
    rng = np.random.default_rng(7 + n)
    dets = _boxes(rng, n, extent=300.0 if n < 10000 else 1500.0, ties=ties)
    want = np.asarray(R.nms_vectorised(dets, thr), np.int64)
    got = nms_gpu_tensor(torch.from_numpy(dets).cuda(), thr).cpu().numpy()
    assert got.shape == want.shape and (got == want).all()
    # size-independent properties: kept boxes are pairwise below the threshold, scores descend
    sc = dets[got, 4]
    assert (np.diff(sc) <= 0).all()


def test_nms_edge_cases():
    from papc_amd.nms import nms_gpu, nms_gpu_tensor
    assert nms_gpu(np.zeros((0, 5), np.float32), 0.5) == []
    same = np.tile(np.array([[10, 10, 20, 20, 0.5]], np.float32), (130, 1))   # identical boxes, tied scores: only the last index
    assert nms_gpu(same, 0.5) == [129]
    far = np.array([[i * 100, 0, i * 100 + 10, 10, 0.1 * i] for i in range(1, 9)], np.float32)   # disjoint: all kept, score order
    assert nms_gpu(far, 0.0) == list(range(7, -1, -1))
    neg = np.array([[0, 0, 10, 10, -1.0], [0, 0, 10, 10, -2.0], [50, 50, 60, 60, 0.0]], np.float32)   # negative scores order
    assert nms_gpu(neg, 0.5) == [2, 0]
    with pytest.raises(Exception):
        nms_gpu_tensor(torch.zeros(4, 5), 0.5)


def _rboxes(rng, n, extent=20.0):
    xy = rng.uniform(0, extent, (n, 2))
    wh = rng.uniform(0.5, 6.0, (n, 2))
    ang = rng.uniform(-np.pi, np.pi, (n, 1))
    return np.concatenate([xy, wh, ang], 1).astype(np.float32)


@pytest.mark.parametrize("criterion", [-1, 0, 1, 2])
def test_rotate_iou_matches_oracle(criterion):
    """The kernel clips (Sutherland-Hodgman, fp64); the oracle is the source's candidate-list + angular-sort routine in its fp32 typing.
    Two different algorithms for the same area: they agree to the source's fp32 rounding (1e-5 absolute on IoU, areas relative) on every
    pair whose edges are not coincident.  Coincident edges (identical boxes at a general angle) are ties between the source's strict
    comparisons -- its result there is rounding noise (the oracle returns anything from 0 to 1) -- and have their geometric value here."""
    from papc_amd.nms import rotate_iou_gpu_eval
    rng = np.random.default_rng(5)
    b, q = _rboxes(rng, 70), _rboxes(rng, 45)
    q[:5] = b[:5]                                            # identical pairs: excluded from the oracle comparison, held to geometry
    q[5, :4], q[5, 4] = b[5, :4], b[5, 4] + np.float32(np.pi / 2)
    want = R.rotate_iou_gpu_eval(b, q, criterion)
    got = rotate_iou_gpu_eval(b, q, criterion)
    assert got.shape == want.shape == (70, 45)
    scale = 1.0 if criterion != 2 else float(want.max())
    general = np.ones((70, 45), bool)
    general[np.arange(5), np.arange(5)] = False
    assert np.abs(got - want)[general].max() <= 1e-5 * scale
    area = (b[:5, 2] * b[:5, 3]).astype(np.float64)
    exact = {-1: np.ones(5), 0: np.ones(5), 1: np.ones(5), 2: area}[criterion]
    assert np.abs(got[np.arange(5), np.arange(5)] - exact).max() <= 2e-6 * max(1.0, float(area.max()))
    if criterion == -1:
        assert (got >= 0).all() and (got <= 1 + 1e-5).all()      # (the clipped area comes from fp32-rounded corners, the box areas from w * l: 1 +- a few 1e-6)
        ax = np.array([[1, 2, 3, 4, 0]], np.float32)
        assert abs(float(rotate_iou_gpu_eval(ax, ax)[0, 0]) - 1.0) < 1e-6


def test_rotate_iou_geometry_properties():
    """Size-independent properties of the intersection area (criterion 2) on 300 x 300 random boxes: symmetric in its arguments, invariant
    under a common rigid motion, bounded by both areas, and equal to the geometric oracle (float64 hull of the candidate points)."""
    from papc_amd.nms import rotate_iou_gpu_eval
    rng = np.random.default_rng(11)
    b, q = _rboxes(rng, 300, 12.0), _rboxes(rng, 300, 12.0)
    a = rotate_iou_gpu_eval(b, q, 2)
    at = rotate_iou_gpu_eval(q, b, 2)
    assert np.abs(a - at.T).max() <= 1e-5
    assert (a <= np.minimum((b[:, 2] * b[:, 3])[:, None], (q[:, 2] * q[:, 3])[None, :]) * (1 + 1e-5) + 1e-6).all() and (a >= 0).all()
    th = np.float32(0.4)
    def move(x):
        y = x.copy()
        c, s = np.cos(th), np.sin(th)
        y[:, 0] = c * x[:, 0] + s * x[:, 1] + 3.0      # the corner rotation of rbbox_to_corners is (x, y) -> (c x + s y, -s x + c y)
        y[:, 1] = -s * x[:, 0] + c * x[:, 1] - 1.0
        y[:, 4] = x[:, 4] + th
        return y.astype(np.float32)
    am = rotate_iou_gpu_eval(move(b), move(q), 2)
    assert np.abs(a - am).max() <= 2e-4                  # (fp32 corners of the moved boxes differ by ~1e-6 relative)
    for n in range(0, 300, 37):
        for k in range(0, 300, 41):
            want = R.convex_quad_inter_area(R.rbbox_to_corners(q[k]), R.rbbox_to_corners(b[n]))
            assert abs(float(a[n, k]) - want) <= 1e-5 * max(1.0, want)


def test_rbbox_iou_and_riou_cc_match_oracle():
    """box_ops.h:23-80 / box_np_ops.py:16-27: corners in, standup pre-test, |P n Q| / |P u Q|; and the one-launch riou_cc."""
    from papc_amd.nms import rbbox_iou, riou_cc
    rng = np.random.default_rng(21)
    b, q = _rboxes(rng, 40, 10.0), _rboxes(rng, 33, 10.0)
    q[:3] = b[:3]
    bc = R.center_to_corner_box2d(b[:, :2], b[:, 2:4], b[:, 4])
    qc = R.center_to_corner_box2d(q[:, :2], q[:, 2:4], q[:, 4])
    su = R.iou_jit(R.corner_to_standup_nd(bc), R.corner_to_standup_nd(qc), eps=0.0)
    for thr in (0.0, 0.2):
        want = R.rbbox_iou(bc, qc, su, thr)
        got = rbbox_iou(bc, qc, su, thr)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5
        assert np.array_equal(got == 0, want == 0) or np.abs(got - want)[(got == 0) != (want == 0)].max() <= 1e-6
        got2 = rbbox_iou(bc, qc, None, thr)              # standup IoU formed on the device
        near = np.abs(su - thr) < 1e-6                   # (a pre-test within rounding of the threshold may fall either way)
        assert np.abs(got2 - want)[~near].max() <= 1e-5
        got3 = riou_cc(b, q, thr)
        want3 = R.riou_cc(b, q, thr)
        assert np.abs(got3 - want3)[~near].max() <= 1e-5
    assert abs(float(got3[0, 0]) - 1.0) < 1e-6 and abs(float(got3[2, 2]) - 1.0) < 1e-6
    assert rbbox_iou(np.zeros((0, 4, 2), np.float32), qc).shape == (0, 33)


def _attribute_keep_list(dets, thr, got, want, ious, band=1e-5):
    """The library's rotated IoU is another algorithm than the source's (Sutherland-Hodgman clipping against the numba routine's vertex sort,
    nms_gpu.py:235-278), equal to 1e-5, so a keep list may differ from the oracle's ONLY through pairs whose IoU is within 1e-5 of the threshold.
    Round 5 forgave any mismatch as soon as SOME pair was that close; here EVERY decision of the library's greedy sweep is attributed: walking
    the boxes in the oracle's score order with the library's own kept set, a box the library KEPT must have no kept predecessor with an oracle
    IoU above thr + band (clearly suppressed), and a box it DROPPED must have a kept predecessor with an oracle IoU above thr - band (plausibly
    suppressed).  Equal lists pass the same walk with a zero band."""
    dets = np.asarray(dets, np.float32)
    n = dets.shape[0]
    order = dets[:, 5].argsort(kind="stable")[::-1]                 # nms_gpu.py:463 (the oracle's and the library's sweep order)
    pos = {int(b): i for i, b in enumerate(order)}
    assert sorted(set(got)) == sorted(got) and all(0 <= g < n for g in got), got
    assert [pos[g] for g in got] == sorted(pos[g] for g in got), "the keep list is not in score order"
    if got == want:
        band = 0.0
    kept = []
    keep_set = set(got)
    thr = float(np.float32(thr))
    for j in range(n):
        box = int(order[j])
        worst = max([ious[(i, j)] for i in kept], default=-1.0)
        if box in keep_set:
            assert worst <= thr + band, "box %d kept although a kept predecessor overlaps it by %.7f > %.7f" % (box, worst, thr)
            kept.append(j)
        else:
            assert worst > thr - band, "box %d dropped although no kept predecessor reaches the threshold (largest IoU %.7f, thr %.7f)" % (box, worst, thr)
    if got != want:
        diff = sorted(set(got) ^ set(want))
        print("rotated NMS: keep lists differ in boxes %s, each attributed to an IoU within %.0e of the threshold" % (diff, band))


@pytest.mark.parametrize("n,thr", [(1, 0.5), (64, 0.3), (65, 0.5), (150, 0.1)])
def test_rotate_nms_matches_oracle(n, thr):
    from papc_amd.nms import rotate_nms_gpu
    rng = np.random.default_rng(100 + n)
    dets = np.concatenate([_rboxes(rng, n, extent=12.0), rng.uniform(0, 1, (n, 1)).astype(np.float32)], 1)
    want, ious = R.rotate_nms_gpu(dets, thr, return_ious=True)
    got = rotate_nms_gpu(dets, thr)
    _attribute_keep_list(dets, thr, got, [int(i) for i in want], ious)


def test_rotate_nms_edge_cases():
    from papc_amd.nms import rotate_nms_gpu, rotate_iou_gpu
    assert rotate_nms_gpu(np.zeros((0, 6), np.float32), 0.5) == []
    same = np.tile(np.array([[3, 3, 2, 1, 0.0, 0.5]], np.float32), (70, 1))       # identical boxes, tied scores
    assert rotate_nms_gpu(same, 0.5) == [69]
    same[:, 4] = 0.7                               # ... at a general angle: exact duplicates suppress each other (the source's IoU is noise there)
    assert rotate_nms_gpu(same, 0.5) == [69]
    far = np.array([[10 * i, 0, 2, 1, 0.3 * i, 0.1 * i] for i in range(1, 6)], np.float32)
    assert rotate_nms_gpu(far, 0.1) == [4, 3, 2, 1, 0]
    assert rotate_iou_gpu(np.zeros((0, 5), np.float32), np.zeros((3, 5), np.float32)).shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------------------
# edges (inputs: tests/detect_cases.py; their ability to fail is checked by tests/test_oracle.py::test_detect_case_tables)
# ---------------------------------------------------------------------------------------------------------------------
def _ints(xs):
    return [int(i) for i in xs]


def test_nms_signed_zero_scores_tie():
    """+0.0 and -0.0 compare equal: to the oracle's stable argsort they are one tie (higher index first), so the score key must not tell
    them apart.  The 130-box input keeps 34 boxes with the zeros tied and 35 with +0.0 ranked first."""
    from papc_amd.nms import nms_gpu
    assert nms_gpu(D.ZERO_PAIR, 0.5) == _ints(R.nms_gpu(D.ZERO_PAIR, 0.5)) == [1]
    swapped = np.ascontiguousarray(D.ZERO_PAIR[::-1])
    assert nms_gpu(swapped, 0.5) == _ints(R.nms_gpu(swapped, 0.5)) == [1]
    dets = D.zero_score_dets()
    assert nms_gpu(dets, D.ZERO_NMS_THR) == _ints(R.nms_gpu(dets, D.ZERO_NMS_THR))


def test_nms_exact_threshold():
    """IoU == thr exactly (0.5 in float32 under the "+1" convention) does not suppress; one float32 step below it does."""
    from papc_amd.nms import nms_gpu
    below = np.nextafter(np.float32(0.5), np.float32(0))
    assert nms_gpu(D.EXACT_THR_PAIR, 0.5) == _ints(R.nms_gpu(D.EXACT_THR_PAIR, 0.5)) == [0, 1]
    assert nms_gpu(D.EXACT_THR_PAIR, below) == _ints(R.nms_gpu(D.EXACT_THR_PAIR, below)) == [0]


def test_rotate_nms_signed_zero_scores_tie():
    from papc_amd.nms import rotate_nms_gpu
    assert rotate_nms_gpu(D.ROTATED_ZERO_PAIR, 0.5) == [1]
    assert rotate_nms_gpu(np.ascontiguousarray(D.ROTATED_ZERO_PAIR[::-1]), 0.5) == [1]


def _corner_iou(ac, bc):
    """the device's IoU of the corner quadrilaterals ac[i], bc[i] (no standup pre-test), pair by pair"""
    from papc_amd.nms import rbbox_iou
    n = len(ac)
    got = rbbox_iou(np.ascontiguousarray(ac), np.ascontiguousarray(bc), standup_iou=np.ones((n, n), np.float32), standup_thresh=0.0)
    return got[np.arange(n), np.arange(n)].astype(np.float64)


def test_rbbox_iou_named_pairs_and_winding():
    """Containment (at KITTI range), coincidence, shared edge / corner, crossings, large angles, on host float32 corners.  The kernel
    works in fp64 on the given corners and rounds once to fp32 (6e-8); the float64 hull oracle is good to 4e-9 here: 1e-6 leaves an order
    of magnitude and still catches a missing vertex or a wrong crossing.  Both argument orders, and every corner order (`wind`)."""
    a, b = D.named_boxes()
    ac, bc = D.corners_of(a), D.corners_of(b)
    want = D.rbbox_iou_pairs(ac, bc)
    got = _corner_iou(ac, bc)
    swapped = _corner_iou(bc, ac)
    for i, name in enumerate(D.NAMED):
        print("%-18s want %.9f got %.9f swapped %.9f" % (name, want[i], got[i], swapped[i]))
    assert np.abs(got - want).max() <= 1e-6 and np.abs(swapped - want).max() <= 1e-6
    for name in D.TOUCHING:
        assert got[D.NAMED.index(name)] < 1e-6 and swapped[D.NAMED.index(name)] < 1e-6
    for ra, rb in ((ac[:, ::-1], bc), (ac, bc[:, ::-1]), (ac[:, ::-1], bc[:, ::-1])):
        assert np.abs(_corner_iou(ra, rb) - got).max() <= 1e-6
        assert np.abs(_corner_iou(rb, ra) - swapped).max() <= 1e-6


def test_rotate_iou_named_pairs_near_origin():
    """The five-vector path (corners formed on the device) on the named pairs near the origin, against the float64 hull."""
    from papc_amd.nms import rotate_iou_gpu_eval
    keep = [i for i, n in enumerate(D.NAMED) if n != "containment"]
    names = [D.NAMED[i] for i in keep]
    a, b = D.named_boxes()
    a, b = a[keep], b[keep]
    want = D.inter_pairs(a, b)
    idx = np.arange(len(a))
    got = rotate_iou_gpu_eval(a, b, 2)[idx, idx].astype(np.float64)
    swapped = rotate_iou_gpu_eval(b, a, 2)[idx, idx].astype(np.float64)
    for i, name in enumerate(names):
        print("%-18s want %.9g got %.9g swapped %.9g" % (name, want[i], got[i], swapped[i]))
    bar = 1e-5 * np.maximum(1.0, want)
    assert (np.abs(got - want) <= bar).all() and (np.abs(swapped - want) <= bar).all()
    for name in D.TOUCHING + ("thin_cross",):
        assert got[names.index(name)] < 1e-5 and swapped[names.index(name)] < 1e-5
    iou = rotate_iou_gpu_eval(a, b, -1)[idx, idx]
    for name in D.COINCIDENT_AXIS_ALIGNED:
        assert abs(float(iou[names.index(name)]) - 1.0) <= 2e-6


def test_rotated_iou_kitti_range():
    """Car-sized boxes 40-70 m out, where a float32 step of a corner is up to 7.6e-6 m.  Host corners: the 1e-6 bar of the named pairs.
    Device corners: cosf / sinf may leave a corner one float32 step from numpy's, which moves a rectangle's edge by that step and the area
    by at most perimeter x step (detect_cases.corner_step_bar)."""
    from papc_amd.nms import rbbox_iou, rotate_iou_gpu_eval
    b, q, bc, qc, iou, inter = D.kitti_reference()
    b, q, bc, qc = b.copy(), q.copy(), bc.copy(), qc.copy()               # (the shared reference is read-only; torch wants writable arrays)
    n, k = len(b), len(q)
    got = rbbox_iou(bc, qc, standup_iou=np.ones((n, k), np.float32), standup_thresh=0.0).astype(np.float64)
    got_t = rbbox_iou(qc, bc, standup_iou=np.ones((k, n), np.float32), standup_thresh=0.0).astype(np.float64)
    r1 = max(np.abs(got - iou).max(), np.abs(got_t.T - iou).max()) / 1e-6
    area = rotate_iou_gpu_eval(b, q, 2).astype(np.float64)
    bar = D.corner_step_bar(b, q, inter)
    r2 = (np.abs(area - inter) / bar).max()
    print("KITTI-range rotated IoU: largest error / bar = %.3f (host corners, bar 1e-6), %.3f (device corners, bar %.2e .. %.2e)"
          % (r1, r2, bar.min(), bar.max()))
    assert r1 <= 1.0
    assert r2 <= 1.0


def test_rotated_zero_area_boxes():
    from papc_amd.nms import rotate_iou_gpu_eval, rotate_nms_gpu
    z, o = D.ZERO_AREA[None], D.ZERO_AREA_OTHER[None]
    for crit in (2, -1):
        assert float(rotate_iou_gpu_eval(z, o, crit)[0, 0]) == 0.0
        assert float(rotate_iou_gpu_eval(o, z, crit)[0, 0]) == 0.0
    v = rotate_iou_gpu_eval(D.ZERO_AREA_SET, D.ZERO_AREA_SET, -1)
    assert v.shape == (3, 3) and not (v > 0).any()                               # 0 / 0: zero or NaN, never an overlap
    assert rotate_nms_gpu(D.ZERO_AREA_NMS, 0.5) == _ints(R.rotate_nms_gpu(D.ZERO_AREA_NMS, 0.5)) == [0, 1, 2]
    # a box shrunk to a point has no interior to clip against: the intersection is empty whichever box is the clipper
    p, h = D.POINT_BOX[None], D.POINT_HOST[None]
    assert float(rotate_iou_gpu_eval(p, h, 2)[0, 0]) == 0.0 and float(rotate_iou_gpu_eval(h, p, 2)[0, 0]) == 0.0
