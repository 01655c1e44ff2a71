"""Inputs of the detection-op edge tests (voxeliser, PointPillarsScatter, NMS, rotated IoU): pure-numpy builders with fixed seeds.
tests/test_gpu_voxel.py and tests/test_gpu_nms.py run them on the device; tests/test_oracle.py::test_detect_case_tables checks, without
a GPU, the conditions that make each input able to fail (a builder that stops meeting them is caught there).  A plain helper module
like tests/torch_ref.py; nothing here touches the library."""
import functools

import numpy as np

from oracle import reference_np as R

f32 = np.float32
KITTI = dict(voxel_size=(0.16, 0.16, 4.0), coors_range=(0, -39.68, -3, 69.12, 39.68, 1))

# ---------------------------------------------------------------------------------------------------------------------
# voxeliser
# ---------------------------------------------------------------------------------------------------------------------
# A grid more than one cell deep in z.  GRID3 is 8 x 10 x 8 cells; GRID3_DISTINCT shortens z to 6 cells so that all three sizes differ
# (a cell index formed with the wrong axis' size then merges or splits cells).
GRID3 = dict(voxel_size=(0.25, 0.2, 0.125), coors_range=(0, -1, -0.5, 2, 1, 0.5))
GRID3_DISTINCT = dict(voxel_size=(0.25, 0.2, 0.125), coors_range=(0, -1, -0.5, 2, 1, 0.25))
GRIDS3 = {"grid8x10x8": GRID3, "grid8x10x6": GRID3_DISTINCT}
GRID3_NDIMS = (3, 4, 6)
GRID3_MAX_POINTS = 4
GRID3_MAX_VOXELS = (20000, 97)


def grid_size(voxel_size, coors_range):
    """point_cloud_ops.py:25 in float32"""
    cr, vs = np.asarray(coors_range, f32), np.asarray(voxel_size, f32)
    return np.round((cr[3:] - cr[:3]) / vs).astype(np.int32)


def cells_f32(pts, voxel_size, coors_range):
    """floor((p - lo) / vs) per axis in float32 (point_cloud_ops.py:35) and the in-range mask"""
    cr, vs = np.asarray(coors_range, f32), np.asarray(voxel_size, f32)
    c = np.floor((pts[:, :3].astype(f32) - cr[:3]) / vs)
    ok = ((c >= 0) & (c < grid_size(voxel_size, coors_range))).all(1)
    return c.astype(np.int64), ok


def grid3_points(ndim, n=1500, seed=17):
    """x, y uniform 15 % beyond the range on both sides, z in [-0.6, 0.6], further columns random; the first three columns do not
    depend on ``ndim``"""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-0.3, 2.3, n), rng.uniform(-1.3, 1.3, n), rng.uniform(-0.6, 0.6, n)], 1)
    extra = rng.uniform(0, 1, (n, 3))
    return np.concatenate([xyz, extra], 1)[:, :ndim].astype(f32)


def lattice_axis(lo, ks):
    """lo + k * 0.16 in float32 for every k, each with its two float32 neighbours"""
    v = f32(lo) + np.asarray(ks, f32) * f32(0.16)
    return np.stack([np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))], 1).reshape(-1).astype(f32)


LATTICE_KX = list(range(0, 428, 7)) + [432]
LATTICE_KY = list(range(0, 496, 9)) + [496]


def lattice_points(seed=23):
    """Points on and one float32 step either side of the KITTI grid's cell boundaries (upper bound included), z = -1."""
    xs = lattice_axis(0, LATTICE_KX)
    ys = lattice_axis(-39.68, LATTICE_KY)[::5]
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    n = X.size
    rng = np.random.default_rng(seed)
    pts = np.stack([X.reshape(-1), Y.reshape(-1), np.full(n, -1.0), rng.uniform(0, 1, n)], 1).astype(f32)
    rng.shuffle(pts)
    return pts


LATTICE_KW = dict(max_points=5, reverse_index=True, max_voxels=20000, **KITTI)


def _cell_point(ix, iy, tag):
    """a point in the middle of KITTI pillar (ix, iy), column 3 = tag"""
    return [0.16 * ix + 0.08, -39.68 + 0.16 * iy + 0.08, -1.0, tag]


def voxel_small_cases():
    """name -> (points, keyword arguments of points_to_voxel)"""
    cases = {}
    same = np.tile(np.array([_cell_point(100, 200, 0)], f32), (300, 1))
    same[:, 3] = np.arange(300)
    cases["same_point_300"] = (same, dict(max_points=35, max_voxels=4))
    cases["one_point"] = (np.array([_cell_point(3, 5, 7)], f32), dict(max_points=5, max_voxels=4))
    a, b = (10, 10), (300, 400)
    order = [a, a, b, a, a, a, b]                      # the second cell opens at index 2: the break; the later points of `a` are dropped
    cases["max_voxels_1"] = (np.array([_cell_point(*c, i) for i, c in enumerate(order)], f32), dict(max_points=5, max_voxels=1))
    outside = np.array([[100.0, 0, 0, 1], [-0.01, 0, 0, 2], [10, 39.68, 0, 3], [10, -40, 0, 4], [10, 0, 1.0, 5], [10, 0, -3.01, 6],
                        [69.12, 0, 0, 7]], f32)
    cases["all_outside"] = (outside, dict(max_points=5, max_voxels=4))
    ten = [(20 * i + 1, 31 * i + 2) for i in range(10)]
    visit = ten + ten + [(431, 495)]
    cut_last = np.array([_cell_point(*c, i) for i, c in enumerate(visit)], f32)
    cases["cut_at_last_point"] = (cut_last, dict(max_points=5, max_voxels=10))
    cases["exactly_max_voxels"] = (cut_last[:-1].copy(), dict(max_points=5, max_voxels=10))
    return {k: (p, dict(reverse_index=True, **kw, **KITTI)) for k, (p, kw) in cases.items()}


@functools.lru_cache(maxsize=None)
def voxel_oracle(key):
    """The oracle's (voxels, coors, num_points) of a named voxeliser input, computed once per session.  key = ("grid3", grid name, ndim,
    reverse, max_voxels) | ("lattice",) | ("small", name)."""
    if key[0] == "grid3":
        _, grid, ndim, reverse, max_voxels = key
        return R.points_to_voxel(grid3_points(ndim), **GRIDS3[grid], max_points=GRID3_MAX_POINTS, reverse_index=reverse, max_voxels=max_voxels)
    if key[0] == "lattice":
        return R.points_to_voxel(lattice_points(), **LATTICE_KW)
    pts, kw = voxel_small_cases()[key[1]]
    return R.points_to_voxel(pts, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# PointPillarsScatter
# ---------------------------------------------------------------------------------------------------------------------
SCATTER_DIMS = dict(B=3, ny=31, nx=27)
SCATTER_C = (1, 7, 64, 65, 130)
SCATTER_P = (1, 3, 501)
SCATTER_SHARED_CELL = (1, 17, 5)                # (batch, y, x) of the cell five pillars share at P = 501


def scatter_outside_kinds(B, ny, nx):
    """(column of coords, value) of every way a row can miss the canvas"""
    return [(0, -1), (0, B), (2, -1), (2, ny), (3, -1), (3, nx)]


def scatter_case(P, C, seed=5):
    """feats [P, C], coords [P, 4] = (batch, z, y, x) with z non-zero (the kernels never read it), grad [B, C, ny, nx].  P = 501: one cell
    holds five pillars and 24 rows (about 5 %) lie outside the canvas, four of each kind; P = 3: rows 0 and 2 share a cell and row 1 is
    outside; P = 1: one row inside."""
    B, ny, nx = SCATTER_DIMS["B"], SCATTER_DIMS["ny"], SCATTER_DIMS["nx"]
    rng = np.random.default_rng(seed + 1000 * P + C)
    coords = np.zeros((P, 4), np.int32)
    coords[:, 0] = rng.integers(0, B, P)
    coords[:, 1] = rng.integers(1, 9, P)
    coords[:, 2] = rng.integers(0, ny, P)
    coords[:, 3] = rng.integers(0, nx, P)
    kinds = scatter_outside_kinds(B, ny, nx)
    if P >= 100:
        rows = rng.permutation(P)
        for r in rows[:5]:
            coords[r, 0], coords[r, 2], coords[r, 3] = SCATTER_SHARED_CELL
        for i, r in enumerate(rows[5:5 + 4 * len(kinds)]):
            col, val = kinds[i % len(kinds)]
            coords[r, col] = val
    elif P == 3:
        coords[2, [0, 2, 3]] = coords[0, [0, 2, 3]]
        coords[1, 0] = B
    feats = rng.normal(size=(P, C)).astype(f32)
    grad = rng.normal(size=(B, C, ny, nx)).astype(f32)
    return feats, coords, grad


def scatter_inside(coords):
    B, ny, nx = SCATTER_DIMS["B"], SCATTER_DIMS["ny"], SCATTER_DIMS["nx"]
    return ((coords[:, 0] >= 0) & (coords[:, 0] < B) & (coords[:, 2] >= 0) & (coords[:, 2] < ny) & (coords[:, 3] >= 0) & (coords[:, 3] < nx))


def scatter_expected(feats, coords, grad):
    """canvas: the oracle on the in-range rows in their original order; gradient: the last in-range pillar of a cell receives
    grad[b, :, y, x], every other row (out-of-range rows included) exactly zero"""
    B, ny, nx = SCATTER_DIMS["B"], SCATTER_DIMS["ny"], SCATTER_DIMS["nx"]
    ok = scatter_inside(coords)
    canvas = R.pillar_scatter(feats[ok], coords[ok], B, ny, nx)
    owner = {}
    for p in np.nonzero(ok)[0]:
        owner[(int(coords[p, 0]), int(coords[p, 2]), int(coords[p, 3]))] = int(p)
    gref = np.zeros_like(feats)
    for (b, y, x), p in owner.items():
        gref[p] = grad[b, :, y, x]
    return canvas, gref


# ---------------------------------------------------------------------------------------------------------------------
# axis-aligned NMS
# ---------------------------------------------------------------------------------------------------------------------
ZERO_PAIR = np.array([[0, 0, 10, 10, +0.0], [0, 0, 10, 10, -0.0]], f32)
ZERO_NMS_THR = 0.3
EXACT_THR_PAIR = np.array([[0, 0, 9, 9, .9], [0, 0, 9, 4, .8]], f32)          # IoU = 50 / (100 + 50 - 50) = 0.5 with the "+1" convention
ROTATED_ZERO_PAIR = np.array([[3, 3, 2, 1, 0, +0.0], [3, 3, 2, 1, 0, -0.0]], f32)


def zero_score_dets(n=130, seed=3):
    """overlapping boxes whose scores are all +0.0 or -0.0: one tie for the oracle (numpy compares the zeros equal)"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 40, (n, 2))
    wh = rng.uniform(5, 30, (n, 2))
    sc = rng.choice(np.array([-0.0, +0.0]), (n, 1))
    return np.concatenate([xy, xy + wh, sc], 1).astype(f32)


def rank_positive_zero_first(dets):
    """the same boxes with every -0.0 score replaced by a small negative one: the order that ranks +0.0 above -0.0"""
    d = np.array(dets, f32)
    neg = (d[:, -1] == 0) & np.signbit(d[:, -1])
    d[neg, -1] = f32(-1e-30)
    return d


# ---------------------------------------------------------------------------------------------------------------------
# rotated IoU
# ---------------------------------------------------------------------------------------------------------------------
_PI = np.pi
NAMED_PAIRS = [                                  # name, (x, y, w, l, angle) of A and of B
    ("containment", [50, -30, 4, 2, .3], [50, -30, 1, .5, 1.1]),
    ("same_axis_aligned", [3, 3, 2, 1, 0], [3, 3, 2, 1, 0]),
    ("quarter_turn", [3, 3, 2, 1, 0], [3, 3, 1, 2, _PI / 2]),
    ("half_turn", [3, 3, 2, 1, 0.7], [3, 3, 2, 1, 0.7 + _PI]),
    ("shared_edge", [0, 0, 2, 2, 0], [2, 0, 2, 2, 0]),
    ("shared_corner", [0, 0, 2, 2, 0], [2, 2, 2, 2, 0]),
    ("cross_45", [0, 0, 2, 2, 0], [0, 0, 2, 2, _PI / 4]),
    ("thin_cross", [0, 0, 1e-3, 10, 0], [0, 0, 10, 1e-3, 0]),
    ("half_overlap", [0, 0, 4, 2, 0], [2, 0, 4, 2, 0]),
    ("large_angles", [1, 2, 3, 2, 11.0], [1.5, 2.5, 2, 3, -9.0]),
]
NAMED = [n for n, _, _ in NAMED_PAIRS]
KNOWN_AREAS = {"cross_45": 8.0 * (np.sqrt(2.0) - 1.0), "half_overlap": 4.0, "same_axis_aligned": 2.0, "quarter_turn": 2.0, "half_turn": 2.0,
               "containment": 0.5, "shared_edge": 0.0, "shared_corner": 0.0, "thin_cross": 1e-6}
TOUCHING = ("shared_edge", "shared_corner")
COINCIDENT_AXIS_ALIGNED = ("same_axis_aligned", "quarter_turn")


def named_boxes():
    a = np.array([p for _, p, _ in NAMED_PAIRS], f32)
    b = np.array([q for _, _, q in NAMED_PAIRS], f32)
    return a, b


def corners_of(boxes):
    """host float32 corners [N, 4, 2] (center_to_corner_box2d)"""
    boxes = np.asarray(boxes, f32)
    return R.center_to_corner_box2d(boxes[:, :2], boxes[:, 2:4], boxes[:, 4]).astype(f32)


def rbbox_iou_pairs(ac, bc):
    """oracle IoU of corner quadrilaterals ac[i] and bc[i], pair by pair (no standup pre-test)"""
    one = np.ones((1, 1), f32)
    return np.array([R.rbbox_iou(ac[i:i + 1], bc[i:i + 1], one, 0.0)[0, 0] for i in range(len(ac))], np.float64)


def inter_pairs(a, b):
    """float64 hull area of the rectangles of a[i] and b[i] on their host float32 corners (rbbox_to_corners)"""
    return np.array([R.convex_quad_inter_area(R.rbbox_to_corners(a[i]), R.rbbox_to_corners(b[i])) for i in range(len(a))], np.float64)


def kitti_boxes(n=60, seed=41):
    """two sets of car-sized boxes around six anchors at KITTI range, where one float32 step of a corner is up to 7.6e-6 m"""
    rng = np.random.default_rng(seed)
    anchors = np.stack([rng.uniform(40, 69, 6), rng.uniform(-39, 39, 6)], 1)

    def one_set():
        ctr = anchors[rng.integers(0, 6, n)] + rng.normal(0, 1, (n, 2))
        dims = rng.normal((3.9, 1.6), (0.4, 0.1), (n, 2))
        ang = rng.uniform(-np.pi, np.pi, (n, 1))
        return np.concatenate([ctr, dims, ang], 1).astype(f32)

    return one_set(), one_set()


@functools.lru_cache(maxsize=None)
def kitti_reference():
    """b, q, host corners bc, qc, the oracle's IoU [60, 60] of the corner quadrilaterals and the float64 hull intersection [60, 60] on the
    rbbox_to_corners corners; computed once per session, treat as read-only"""
    b, q = kitti_boxes()
    bc, qc = corners_of(b), corners_of(q)
    iou = R.rbbox_iou(bc, qc, np.ones((len(b), len(q)), f32), 0.0).astype(np.float64)
    rb = [R.rbbox_to_corners(x) for x in b]
    rq = [R.rbbox_to_corners(x) for x in q]
    inter = np.array([[R.convex_quad_inter_area(rq[k], rb[n]) for k in range(len(q))] for n in range(len(b))], np.float64)
    for arr in (b, q, bc, qc, iou, inter):
        arr.setflags(write=False)
    return b, q, bc, qc, iou, inter


def corner_step_bar(b, q, want):
    """Bar for the intersection area when the DEVICE forms the corners: its cosf / sinf may leave a corner coordinate one float32 step from
    numpy's, which changes a rectangle by at most perimeter x step; the factor 2 covers both coordinates moving.
    1e-6 max(1, want) + 2 (perimeter_A + perimeter_B) spacing(max |corner coordinate| of the pair)"""
    per_b = 2.0 * (b[:, 2].astype(np.float64) + b[:, 3])
    per_q = 2.0 * (q[:, 2].astype(np.float64) + q[:, 3])
    mb = np.abs(np.stack([R.rbbox_to_corners(x) for x in b])).max(1)
    mq = np.abs(np.stack([R.rbbox_to_corners(x) for x in q])).max(1)
    step = np.spacing(np.maximum(mb[:, None], mq[None, :]).astype(f32)).astype(np.float64)
    return 1e-6 * np.maximum(1.0, want) + 2.0 * (per_b[:, None] + per_q[None, :]) * step


ZERO_AREA = np.array([0, 0, 0, 2, 0], f32)
ZERO_AREA_OTHER = np.array([0, 0, 2, 2, .2], f32)
ZERO_AREA_SET = np.array([[0, 0, 0, 2, 0], [3, 3, 0, 0, 0], [0, 0, 2, 0, .4]], f32)
ZERO_AREA_NMS = np.array([[3, 3, 0, 1, .3, .9], [3, 3, 2, 1, .3, .8], [3, 3, 0, 0, 0, .7]], f32)
# a box shrunk to a point inside a proper box: the intersection of anything with a set of zero area has zero area, in either argument order
POINT_BOX = np.array([3, 3, 0, 0, 0], f32)
POINT_HOST = np.array([3, 3, 2, 1, .3], f32)
