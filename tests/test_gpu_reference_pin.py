"""The HIP path held to the REFERENCE'S OWN model code, executed: tests/golden/ref_*.npz (tests/golden/make_reference_golden.py ran the reference's
program text on the paddle stand-in and recorded what came out).  Reads only tests/golden/.

The fixtures' inputs meet the generator's conditions (every squared distance a relative 1e-5 off r^2, every farthest-point winner a relative
1e-5 ahead, neighbour distances separated by as much), so any correct fp32 evaluation order yields the recorded indices: an index
mismatch here is a finding, not rounding.  Bars: indices exact; float32-mode distance rows bit-equal; standalone SA / FP layers 1e-5; the
voxeliser bit-exact; per model the head input, the running statistics and the eval-mode logits at 2e-4 (the fp32 chain against float64,
DESIGN section 4).  The recorded forwards draw no dropout mask (p = 0 on both sides): the device draws its own masks."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn

from papc_amd import functional as F_
from papc_amd import layers as PL
from tests.ref_fixtures import MODELS, SEG_STRIDE, gold, sa_weights, seeded_product
from tests.util import assert_close, fps_lattice

pytestmark = pytest.mark.gpu
BAR = 2e-4


@pytest.fixture(scope="module")
def lay():
    return gold("ref_layers")


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _feats(cloud):
    return np.ascontiguousarray((np.transpose(cloud, (0, 2, 1))[:, ::-1, :] * 2.0 + 0.25).astype(np.float32))   # [B, 3, N], as the generator's


# ---------------------------------------------------------------------------------------------------------------------------------------
# layer functions
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_square_distance_rows_bit_equal(dev, lay):
    cloud = lay["cloud"]
    got = _np(F_.square_distance(_dev(cloud[:, :64], dev), _dev(cloud[:, 100:200], dev)))
    ref = lay["sqdist_32"]
    diff = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    print("[pin] square_distance: %d of %d entries differ from the float32-mode run, max %d ulp" % (int((diff > 0).sum()), diff.size, int(diff.max())))
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))


def test_fps_indices(dev, lay):
    cloud = _dev(lay["cloud"], dev)
    got = F_.farthest_point_sample(cloud, 128, _dev(lay["start1"].astype(np.int64), dev))
    assert got.dtype == torch.int64 and np.array_equal(_np(got), lay["fps_cloud"].astype(np.int64))
    latt = fps_lattice(2, int(lay["lattice_seed"]))[:, :int(lay["lattice_n"])]
    got = F_.farthest_point_sample(_dev(latt, dev), 64, _dev(lay["lattice_start"].astype(np.int64), dev))
    assert np.array_equal(_np(got), lay["fps_lattice"].astype(np.int64))            # every iteration ties: only the first-maximum rule decides


@pytest.mark.parametrize("key,radius,nsample", [("ball_r02", 0.2, 32), ("ball_r005", 0.05, 16)])
def test_ball_query_indices(dev, lay, key, radius, nsample):
    cloud = lay["cloud"]
    q = cloud[np.arange(2)[:, None], lay["fps_cloud"].astype(np.int64)] if key == "ball_r02" else lay["queries"]
    got = F_.query_ball_point(radius, nsample, _dev(cloud, dev), _dev(q, dev))
    assert got.dtype == torch.int64 and np.array_equal(_np(got), lay[key].astype(np.int64))     # (r = 0.05: some queries hit nothing and keep N)


def test_sample_and_group(dev, lay):
    g = gold("ref_group")
    cloud = lay["cloud"]
    feats = np.ascontiguousarray(np.transpose(_feats(cloud), (0, 2, 1)))
    new_xyz, new_points, grouped_xyz, fps = F_.sample_and_group(32, 0.2, 16, _dev(cloud, dev), _dev(feats, dev), returnfps=True,
                                                                start_idx=_dev(lay["start1"].astype(np.int64), dev))
    assert np.array_equal(_np(fps), g["sg_fps"].astype(np.int64))
    assert np.array_equal(_np(new_xyz), g["sg_new_xyz_32"])
    assert np.array_equal(_np(new_points), g["sg_new_points_32"])          # [centred xyz, features]: gathers and one fp32 subtraction, bit-equal
    assert_close(_np(new_points), g["sg_new_points_64"], rel=1e-6, what="sample_and_group vs the float64 run")
    a, b = F_.sample_and_group_all(_dev(cloud[:, :128], dev), _dev(feats[:, :128], dev))
    assert np.array_equal(_np(a), g["sga_new_xyz_32"]) and np.array_equal(_np(b), g["sga_new_points_32"])


def _load_stack(layer, prefix, chans, seed, dev):
    with torch.no_grad():
        for i, (w, b, ga, be) in enumerate(sa_weights(prefix, chans, seed)):
            layer.mlp_convs[i].weight.copy_(torch.from_numpy(w).reshape(layer.mlp_convs[i].weight.shape))
            layer.mlp_convs[i].bias.copy_(torch.from_numpy(b))
            layer.mlp_bns[i].weight.copy_(torch.from_numpy(ga))
            layer.mlp_bns[i].bias.copy_(torch.from_numpy(be))
    return layer.to(dev).train()


def test_set_abstraction_layer(dev, lay):
    g = gold("ref_group")
    cloud = lay["cloud"]
    sa = _load_stack(PL.PointNetSetAbstraction(32, 0.2, 16, 6, [16, 32], False), "sa", [6, 16, 32], int(lay["weight_seed"]), dev)
    planar = np.ascontiguousarray(np.transpose(cloud, (0, 2, 1)))
    with torch.no_grad():
        new_xyz, out = sa(_dev(planar, dev), _dev(_feats(cloud), dev), _dev(lay["start1"].astype(np.int64), dev))
    assert np.array_equal(_np(new_xyz), g["sa_new_xyz_32"])
    assert_close(_np(out), g["sa_new_points_64"], rel=1e-5, what="SA layer vs the reference's float64 run")
    assert_close(_np(sa.mlp_bns[0].running_mean), g["sa_mean0_64"], rel=1e-5, what="SA layer running mean")
    assert_close(_np(sa.mlp_bns[0].running_var), g["sa_var0_64"], rel=1e-5, what="SA layer running variance")


def test_three_nn_and_feature_propagation(dev, lay):
    z = gold("ref_fp")
    cloud = lay["cloud"]
    xyz1, xyz2 = cloud[np.arange(2)[:, None], z["fp_query_idx"].astype(np.int64)], cloud[:, 300:364]
    d3, idx3, w3 = F_.three_nn(_dev(xyz1, dev), _dev(xyz2, dev))
    assert np.array_equal(_np(d3).view(np.int32), z["fp_s64_dist3_32"].view(np.int32))        # the float32-mode distance rows: bit-equal
    d64 = np.sort(((xyz1.astype(np.float64)[:, :, None] - xyz2.astype(np.float64)[:, None]) ** 2).sum(-1), -1)[:, :, :3]
    assert_close(z["fp_s64_dist3"], d64, rel=1e-12, what="recorded float64 distances are the three smallest")
    true_idx = np.argsort(((xyz1.astype(np.float64)[:, :, None] - xyz2.astype(np.float64)[:, None]) ** 2).sum(-1), -1, kind="stable")[:, :, :3]
    assert np.array_equal(_np(idx3).astype(np.int64), true_idx)                               # three_nn's own indices: the true neighbours
    rec = 1.0 / (z["fp_s64_dist3"] + 1e-8)
    assert_close(_np(w3), rec / rec.sum(-1, keepdims=True), rel=1e-5, what="three_nn weights vs the recorded float64 distances")
    p2 = np.ascontiguousarray(np.transpose(z["fp_points2"], (0, 2, 1)))
    ref_idx = z["fp_s64_idx3"].astype(np.int64)                                               # the reference's sort-then-argsort neighbours: 0, 1, 2
    got = _np(F_.three_interpolate(_dev(p2, dev), _dev(ref_idx.astype(np.int32), dev), w3))
    w64 = rec / rec.sum(-1, keepdims=True)
    want = (p2.astype(np.float64)[np.arange(2)[:, None, None], ref_idx] * w64[..., None]).sum(2)
    assert_close(got, want, rel=1e-5, what="three_interpolate on the recorded neighbours")
    for tag, sl in (("s64", slice(None)), ("s1", slice(0, 1))):
        fp = _load_stack(PL.PointNetFeaturePropagation(22, [32, 16]), "fp", [22, 32, 16], int(lay["weight_seed"]), dev)
        with torch.no_grad():
            out = fp(_dev(np.transpose(xyz1, (0, 2, 1)), dev), _dev(np.transpose(xyz2, (0, 2, 1))[:, :, sl], dev), _dev(z["fp_points1"], dev),
                     _dev(z["fp_points2"][:, :, sl], dev))
        assert_close(_np(out), z["fp_%s_out" % tag], rel=1e-5, what="FP layer %s vs the reference's float64 run" % tag)
        assert_close(_np(fp.mlp_bns[0].running_var), z["fp_%s_var0" % tag], rel=1e-5, what="FP layer %s running variance" % tag)


def test_voxeliser_bit_exact(dev):
    from papc_amd.voxel import points_to_voxel
    from tests import detect_cases as D
    z = gold("ref_voxel")
    cases = {"small_" + k: v for k, v in D.voxel_small_cases().items()}
    cases["lattice"] = (D.lattice_points(), dict(D.LATTICE_KW))
    for grid, g in D.GRIDS3.items():
        for mv in D.GRID3_MAX_VOXELS:
            cases["grid3_%s_mv%d" % (grid, mv)] = (D.grid3_points(3), dict(max_points=D.GRID3_MAX_POINTS, reverse_index=True, max_voxels=mv, **g))
    assert sorted(cases) == sorted(str(s) for s in z["case_names"])
    for name, (pts, kw) in cases.items():
        v, c, n = (_np(t) for t in points_to_voxel(_dev(np.asarray(pts, np.float32), dev), **kw))
        assert len(v) == int(z[name + "_n"]), name
        assert np.array_equal(c, z[name + "_coors"]) and np.array_equal(n, z[name + "_num"]), name
        assert zlib.crc32(np.ascontiguousarray(v).tobytes()) == int(z[name + "_voxels_crc"]), name


# ---------------------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------------------
def _inputs(name, z, lay, dev):
    """(what the model's forward takes, keyword arguments)"""
    if name == "kdnet":
        kd = gold("kdtree_n1024")
        return (([_dev(z["points"], dev), [kd["split_%d" % i].astype(np.int64) for i in range(10)]],), {})
    if name == "voxnet":
        return ((_dev(np.unpackbits(z["grid_bits"]).reshape(3, 1, 32, 32, 32).astype(np.float32), dev),), {})
    x = _dev(np.transpose(lay["cloud"], (0, 2, 1)), dev)
    if name in ("basic_clas", "pointnet_clas"):
        return ((x,), {})
    starts = dict(start_idx=(_dev(lay["start1"].astype(np.int64), dev), _dev(lay["start2"].astype(np.int64), dev)))
    if name == "ssg_seg":
        return (([x, _dev(lay["seg_labels"], dev)],), starts)
    return ((x,), starts)


def _model(name, dev):
    model, z = seeded_product(name)
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    return model.to(dev), z


def _head_input(name, model, args, kw, monkeypatch):
    """the tensor entering the model's head, from a second seeded copy of the model: the classifiers' heads are fused launches that call no
    module, so this copy runs them through the modules (papc_amd.models._FUSED_HEAD off) with a hook on the head's first one; the
    segmenter and VoxNet are taken apart at their public layer calls (KDNet: test_kdnet_head_input)"""
    from papc_amd import models as M
    model.train()
    if name in ("ssg_clas", "msg_clas", "basic_clas", "pointnet_clas"):
        monkeypatch.setattr(M, "_FUSED_HEAD", False)
        got = []
        head = model.fc1 if hasattr(model, "fc1") else model.fc

        def tap(m, a):
            got.append(a[0].detach().clone())

        h = head.register_forward_pre_hook(tap)
        with torch.no_grad():
            model(*args, **kw)
        h.remove()
        return got[0]
    if name == "voxnet":
        from papc_amd import voxnet
        b = model.backbone
        with torch.no_grad():
            return voxnet.voxconv_backbone(args[0], b[0], b[1], b[3], True)
    assert name == "ssg_seg"
    xyz, labels = args[0]
    B, _, N = xyz.shape
    with torch.no_grad():
        (l1_xyz, l1_p), (l2_xyz, l2_p), (l3_xyz, l3_p) = model._encode(xyz, xyz, kw["start_idx"])
        l2_p = model.fp3(l2_xyz, l3_xyz, l2_p, l3_p)
        l1_p = model.fp2(l1_xyz, l2_xyz, l1_p, l2_p)
        onehot = M.Categorical(labels, model.num_classes).to(xyz.device).reshape(B, model.num_classes, 1).expand(B, model.num_classes, N)
        return model.fp1(xyz, l1_xyz, torch.cat([onehot, xyz, xyz], 1), l1_p)


def _norm(model, ref_name):
    """this project's module for a norm the reference names (PointNet_Basic_Clas keeps its own container names)"""
    names = getattr(type(model), "reference_names", None) or {}
    inv = {v: k for k, v in names.items()}
    own = inv.get(ref_name, ref_name)
    return dict(model.named_modules())[own]


def _elem(z, key):
    """the elementwise side of the model-level bar: assert_close's 100 x the max-norm bar, but never tighter than 3 x what the reference ITSELF
    deviates from its float64 run when it computes in float32 (recorded by the generator as own32_*).  That matters for the segmenter
    alone: its feature-propagation levels weight by 1 / (d + 1e-8) with d = -2 a.b + |a|^2 + |b|^2, and a level's centroids are among its
    queries, so d is 0 exactly in float64 and +-3e-8 of cancellation noise in ANY float32 evaluation: the reference's own float32 mode is
    1.1e-4 (max-norm) / 2.8e-2 (elementwise) from its float64 run at the head input.  The max-norm bar stays 2e-4 for every model."""
    return max(100.0 * BAR, 3.0 * float(z["own32_" + key][1]))


@pytest.mark.parametrize("name", MODELS)
def test_model_against_the_reference_run(dev, lay, name, monkeypatch):
    model, z = _model(name, dev)
    args, kw = _inputs(name, z, lay, dev)
    # sampling indices of both levels, exact
    if "fps_0" in z.files:
        cloud = lay["cloud"]
        xyz = args[0][0] if name == "ssg_seg" else args[0]
        with torch.no_grad():
            p1 = model.sa1.sample(xyz, kw["start_idx"][0])
            p2 = model.sa2.sample(p1[0].transpose(1, 2), kw["start_idx"][1])
        ar = np.arange(2)[:, None]
        l1 = cloud[ar, z["fps_0"].astype(np.int64)]
        assert np.array_equal(_np(p1[0]), l1), "level-1 centroids are not the recorded farthest points"
        assert np.array_equal(_np(p2[0]), l1[ar, z["fps_1"].astype(np.int64)]), "level-2 centroids are not the recorded farthest points"
        n1 = len(model.sa1.radius_list) if hasattr(model.sa1, "radius_list") else 1
        n2 = len(model.sa2.radius_list) if hasattr(model.sa2, "radius_list") else 1
        idxs = list(p1[1:1 + n1]) + list(p2[1:1 + n2])
        assert len(idxs) == sum(1 for k in z.files if k.endswith("_crc"))
        for i, idx in enumerate(idxs):
            got = _np(idx).astype(np.int16)
            radius, nsample, n, s = z["ball_%d_meta" % i]
            assert got.shape == (2, int(s), int(nsample)), (i, got.shape)
            assert np.array_equal(got[:, ::4], z["ball_%d_rows" % i]), "ball query %d (r = %g): indices differ" % (i, radius)
            assert zlib.crc32(np.ascontiguousarray(got).tobytes()) == int(z["ball_%d_crc" % i]), "ball query %d (r = %g): indices differ" % (i, radius)
    # one train-mode forward: running statistics of the first and the last norm
    model.train()
    with torch.no_grad():
        model(*args, **kw)
    for tag in ("first", "last"):
        if tag + "_norm" in z.files:
            bn = _norm(model, str(z[tag + "_norm"][0]))
            assert_close(_np(bn.running_mean), z[tag + "_mean"], rel=BAR, what="%s %s running mean" % (name, z[tag + "_norm"][0]))
            assert_close(_np(bn.running_var), z[tag + "_var"], rel=BAR, what="%s %s running variance" % (name, z[tag + "_norm"][0]))
    # eval-mode logits on the updated statistics
    model.eval()
    with torch.no_grad():
        ev = _np(model(*args, **kw))
    assert_close(ev[:, ::SEG_STRIDE] if name == "ssg_seg" else ev, z["eval_logits"], rel=BAR, what=name + " eval logits", elem=_elem(z, "eval_logits"))
    if name == "kdnet":
        return          # (its head input: test_kdnet_head_input)
    # the tensor entering the head
    twin, _ = _model(name, dev)
    h = _np(_head_input(name, twin, args, kw, monkeypatch))
    if name == "ssg_seg":
        h = h[..., ::SEG_STRIDE]
    assert_close(h.reshape(z["head_in"].shape), z["head_in"], rel=BAR, what=name + " head input", elem=_elem(z, "head_in"))


def test_kdnet_head_input(dev, lay):
    """KDNet's head is one Linear(128, 10) on the device's row kernel and calls no module: its input is read through the head itself, with
    the weight set to 10-row slices of the 128 x 128 identity, thirteen forwards"""
    model, z = _model("kdnet", dev)
    args, _ = _inputs("kdnet", z, lay, dev)
    model.train()
    cols = []
    eye = torch.eye(128, device=dev)
    with torch.no_grad():
        model.fc.bias.zero_()
        for lo in list(range(0, 120, 10)) + [118]:
            model.fc.weight.copy_(eye[lo:lo + 10])
            cols.append((lo, model(*args)))
    h = torch.zeros(2, 128, device=dev)
    for lo, c in cols:
        h[:, lo:lo + 10] = c
    assert_close(_np(h), z["head_in"], rel=BAR, what="kdnet head input", elem=_elem(z, "head_in"))


@pytest.mark.parametrize("name", ["ssg_clas", "ssg_seg"])
def test_reference_quirks_gradient_holders(dev, lay, name):
    """reference_quirks=True: after logits.sum().backward() exactly the reference's trainable parameters hold a gradient (the layers it keeps
    in plain lists are frozen here; in the reference those behind an index_points cut receive none and the others are never stepped)"""
    from papc_amd import checkpoint
    model, z = seeded_product(name, reference_quirks=True)
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    model = model.to(dev).train()
    args, kw = _inputs(name, z, lay, dev)
    model(*args, **kw).sum().backward()
    got = sorted(checkpoint._to_reference_name(n, model) for n, p in model.named_parameters() if p.grad is not None)
    assert got == sorted(str(s) for s in z["param_names"])
    assert set(got) <= set(str(s) for s in z["grad_names"])
