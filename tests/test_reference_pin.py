"""The oracles held to the REFERENCE'S OWN model code, executed (CPU).  tests/golden/ref_*.npz hold what the reference's program text
computed on the paddle stand-in (tests/golden/make_reference_golden.py); this file reads only those fixtures.  Compared against them:
oracle/reference_np.py and oracle/torch_cpu_reference.py (layer functions, SA / FP layers, the models they state), the float64 twins under
tests/*_ref.py (PointNet_Clas, KDNet, VoxNet), papc_amd/checkpoint.py's name mapping, and which parameters this project's models train.

Bars.  Indices: exact.  float64 against float64 (torch_cpu_reference run in double, the twins): 1e-9 of max|ref| -- both sides are float64 and
the sums run over at most ~1e5 terms, so this leaves about three decades over what summation order explains; a structural error (a swapped
concat, [in, out] read as [out, in], the wrong momentum side) is 1e-3 or more.  oracle/reference_np.py gathers and centres coordinates in
float32 by design (its canonical fp32 chain), so its float64 path differs from the float64-mode fixture by that input rounding: it is held at
the per-layer 1e-5 bar, and bit for bit against the float32-mode fixture wherever it does no accumulation."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import reference_np as R
from oracle import torch_cpu_reference as TR
from tests.ref_fixtures import MODELS, SEG_STRIDE, gold, make_product, recorded_state, seeded_product, sa_weights as _sa_weights
from tests.util import assert_close, fps_lattice

F64 = 1e-9


@pytest.fixture(scope="module")
def lay():
    return gold("ref_layers")


def close64(got, ref, what):
    return assert_close(got, ref, rel=F64, what=what, elem=1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------------
# layer functions
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_square_distance_float32_mode_is_the_canonical_chain(lay):
    """The float32-mode rows of the reference's -2 a.b + |a|^2 + |b|^2 (torch's K = 3 matmul on the host that generated the fixture; the
    generator refuses to write anything else) are the C oracle's canonical k-ordered chain, bit for bit.  torch's matmul on ANOTHER host
    need not be (measured on one: 67 of 12 800 entries off, up to 32 ulp of small, cancelled values), so the torch-CPU port is held to what
    any fp32 evaluation must meet here: a few ulp(1) of the float64 run, every term being below 1."""
    cloud = lay["cloud"]
    src, dst = cloud[:, :64], cloud[:, 100:200]
    ref = lay["sqdist_32"]
    ulp1 = 2.0 ** -24
    for name, got in (("reference_np.square_distance", R.square_distance(src, dst)), ("square_distance_c", R.square_distance_c(src, dst)),
                      ("torch_cpu_reference", TR.square_distance(torch.from_numpy(src), torch.from_numpy(dst)).numpy())):
        diff = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        print("[pin] square_distance %s: %d of %d entries differ, max %d ulp" % (name, int((diff > 0).sum()), diff.size, int(diff.max())))
        if name != "torch_cpu_reference":
            assert np.array_equal(got.view(np.int32), ref.view(np.int32)), name
        assert np.abs(got.astype(np.float64) - lay["sqdist_64"]).max() < 4 * ulp1, name
    assert np.abs(ref.astype(np.float64) - lay["sqdist_64"]).max() < 4 * ulp1


def test_fps_indices(lay):
    cloud, start = lay["cloud"], lay["start1"].astype(np.int64)
    ref = lay["fps_cloud"].astype(np.int64)
    assert np.array_equal(R.farthest_point_sample(cloud, 128, start), ref)
    assert np.array_equal(R.farthest_point_sample_literal(cloud, 128, start), ref)
    assert np.array_equal(TR.farthest_point_sample(torch.from_numpy(cloud), 128, start).numpy(), ref)
    latt = fps_lattice(2, int(lay["lattice_seed"]))[:, :int(lay["lattice_n"])]
    ls = lay["lattice_start"].astype(np.int64)
    ref = lay["fps_lattice"].astype(np.int64)
    assert np.array_equal(R.farthest_point_sample(latt, 64, ls), ref)                # every iteration ties: only the first-maximum rule decides
    assert np.array_equal(R.farthest_point_sample_literal(latt, 64, ls), ref)
    assert np.array_equal(TR.farthest_point_sample(torch.from_numpy(latt), 64, ls).numpy(), ref)
    assert np.array_equal(ref[:, 0], ls) and len(set(ref[0].tolist())) == 64


@pytest.mark.parametrize("key,radius,nsample", [("ball_r02", 0.2, 32), ("ball_r005", 0.05, 16)])
def test_ball_query_indices(lay, key, radius, nsample):
    cloud = lay["cloud"]
    if key == "ball_r02":
        q = cloud[np.arange(2)[:, None], lay["fps_cloud"].astype(np.int64)]
    else:
        q = lay["queries"]
    ref = lay[key].astype(np.int64)
    N = cloud.shape[1]
    if key == "ball_r005":
        empty = (ref == N).all(-1)
        assert empty.any() and not empty.all() and ((ref == N).any(-1) == empty).all()   # a query without a hit keeps N in every slot
    assert (ref[:, :, 1:] == ref[:, :, :1]).any()                                          # ... and padding with the first hit occurs
    assert np.array_equal(R.query_ball_point(radius, nsample, cloud, q), ref)
    assert np.array_equal(R.query_ball_point_literal(radius, nsample, cloud, q), ref)
    assert np.array_equal(TR.query_ball_point(radius, nsample, torch.from_numpy(cloud), torch.from_numpy(q)).numpy(), ref)


def _feats(cloud):
    return np.ascontiguousarray((np.transpose(cloud, (0, 2, 1))[:, ::-1, :] * 2.0 + 0.25).astype(np.float32))   # [B, 3, N], as the generator's


def test_sample_and_group(lay):
    g = gold("ref_group")
    cloud, start = lay["cloud"], lay["start1"].astype(np.int64)
    feats = np.transpose(_feats(cloud), (0, 2, 1))
    new_xyz, new_points, _, fps = R.sample_and_group(32, 0.2, 16, cloud, feats, start, returnfps=True)
    assert np.array_equal(fps, g["sg_fps"]) and np.array_equal(fps, lay["fps_cloud"][:, :32])
    assert np.array_equal(new_xyz, g["sg_new_xyz_32"])
    assert np.array_equal(new_points, g["sg_new_points_32"])                 # [centred xyz, features]: gathers and one fp32 subtraction, bit-equal
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    nx, grouped, fi, _ = TR.sample_and_group(32, 0.2, 16, t(cloud), t(feats), start)
    assert np.array_equal(fi.numpy().astype(np.int64), g["sg_fps"])
    close64(grouped.numpy(), g["sg_new_points_64"], "sample_and_group torch_cpu_reference float64")
    a, b = R.sample_and_group_all(cloud[:, :128], feats[:, :128])
    assert np.array_equal(a, g["sga_new_xyz_32"]) and np.array_equal(b, g["sga_new_points_32"])
    assert tuple(b.shape) == (2, 1, 128, 6) and np.array_equal(b[:, 0, :, :3], cloud[:, :128])


def test_set_abstraction_layer(lay):
    """PointNetSetAbstraction(32, 0.2, 16, 6, [16, 32], False): reference_np at the per-layer 1e-5 bar (its grouping is fp32), the torch
    transliteration in double at 1e-9"""
    g = gold("ref_group")
    cloud, start = lay["cloud"], lay["start1"].astype(np.int64)
    seed = int(lay["weight_seed"])
    ws = _sa_weights("sa", [6, 16, 32], seed)
    planar, feats = np.ascontiguousarray(np.transpose(cloud, (0, 2, 1))), _feats(cloud)
    sa = R.PointNetSetAbstraction(32, 0.2, 16, 6, [16, 32], False, ws)
    new_xyz, out = sa.forward(planar, feats, start, f64=True)
    assert np.array_equal(new_xyz, g["sa_new_xyz_32"])
    assert_close(out, g["sa_new_points_64"], rel=1e-5, what="SA layer reference_np f64 path")
    _, out32 = sa.forward(planar, feats, start, f64=False)
    assert_close(out32, g["sa_new_points_64"], rel=1e-5, what="SA layer reference_np fp32 chain")
    m = TR.SetAbstraction(32, 0.2, 16, 6, [16, 32], False).double()
    with torch.no_grad():
        for i, (w, b, ga, be) in enumerate(ws):
            m.convs[i].weight.copy_(torch.from_numpy(w).reshape(m.convs[i].weight.shape))
            m.convs[i].bias.copy_(torch.from_numpy(b))
            m.bns[i].weight.copy_(torch.from_numpy(ga))
            m.bns[i].bias.copy_(torch.from_numpy(be))
    paddle_running_stats(m)
    _, o = m(torch.from_numpy(planar.astype(np.float64)), torch.from_numpy(feats.astype(np.float64)), start)
    settle_running_stats(m)
    close64(o.detach().numpy(), g["sa_new_points_64"], "SA layer torch_cpu_reference float64")
    close64(m.bns[0].running_mean.numpy(), g["sa_mean0_64"], "SA layer running mean")
    close64(m.bns[0].running_var.numpy(), g["sa_var0_64"], "SA layer running variance (biased, momentum 0.9)")


def test_feature_propagation():
    z, lay = gold("ref_fp"), gold("ref_layers")
    cloud, seed = lay["cloud"], int(lay["weight_seed"])
    xyz1 = np.ascontiguousarray(np.transpose(cloud[np.arange(2)[:, None], z["fp_query_idx"].astype(np.int64)], (0, 2, 1)))
    xyz2 = np.ascontiguousarray(np.transpose(cloud[:, 300:364], (0, 2, 1)))
    p1, p2 = z["fp_points1"], z["fp_points2"]
    ws = _sa_weights("fp", [22, 32, 16], seed)
    # the sort-then-argsort quirk: the reference's neighbours are 0, 1, 2 for every query, weighted by the three smallest distances
    assert np.array_equal(z["fp_s64_idx3"], np.broadcast_to(np.arange(3, dtype=np.int16), z["fp_s64_idx3"].shape))
    d3, idx, w3 = R.three_nn_literal(np.transpose(xyz1, (0, 2, 1)), np.transpose(xyz2, (0, 2, 1)))
    assert np.array_equal(idx, z["fp_s64_idx3"].astype(np.int64))
    assert np.array_equal(d3.view(np.int32), z["fp_s64_dist3_32"].view(np.int32))          # the float32-mode rows: bit-equal
    assert_close(d3, z["fp_s64_dist3"], rel=1e-6, what="three_nn distances fp32 vs float64 run")
    rec = 1.0 / (z["fp_s64_dist3"] + 1e-8)
    assert_close(w3, rec / rec.sum(-1, keepdims=True), rel=1e-5, what="three_nn weights from the recorded distances")
    for tag, x2, q2 in (("s64", xyz2, p2), ("s1", xyz2[:, :, :1], p2[:, :, :1])):
        fp = R.PointNetFeaturePropagation(22, [32, 16], ws)
        if tag == "s64":     # reference_np's neighbour distances are fp32 by design (bit-equal to the float32-mode run above): its float32-mode twin
            assert_close(fp.forward(xyz1, x2, p1, q2, f64=False), z["fp_s64_out_32"], rel=1e-5, what="FP s64 reference_np vs the float32-mode run")
        else:
            assert_close(fp.forward(xyz1, x2, p1, q2, f64=True), z["fp_s1_out"], rel=1e-5, what="FP s1 reference_np")
        m = TR.FeaturePropagation(22, [32, 16]).double()
        with torch.no_grad():
            for i, (w, b, ga, be) in enumerate(ws):
                m.convs[i].weight.copy_(torch.from_numpy(w).reshape(m.convs[i].weight.shape))
                m.convs[i].bias.copy_(torch.from_numpy(b))
                m.bns[i].weight.copy_(torch.from_numpy(ga))
                m.bns[i].bias.copy_(torch.from_numpy(be))
        paddle_running_stats(m)
        t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
        close64(m(t(xyz1), t(x2), t(p1), t(q2)).detach().numpy(), z["fp_%s_out" % tag], "FP %s torch_cpu_reference float64" % tag)
        settle_running_stats(m)
        close64(m.bns[0].running_var.numpy(), z["fp_%s_var0" % tag], "FP %s running variance" % tag)


def test_voxeliser_matches_the_reference_binary():
    """points_to_voxel<float, 3> of the reference's C++ header, recorded on tests/detect_cases.py's inputs: the oracle's loop, bit for bit"""
    from tests import detect_cases as D
    z = gold("ref_voxel")
    cases = {"small_" + k: v for k, v in D.voxel_small_cases().items()}
    cases["lattice"] = (D.lattice_points(), dict(D.LATTICE_KW))
    for grid, g in D.GRIDS3.items():
        for mv in D.GRID3_MAX_VOXELS:
            cases["grid3_%s_mv%d" % (grid, mv)] = (D.grid3_points(3), dict(max_points=D.GRID3_MAX_POINTS, reverse_index=True, max_voxels=mv, **g))
    assert sorted(cases) == sorted(str(s) for s in z["case_names"])
    assert int(z["small_max_voxels_1_n"]) == 1 and int(z["small_all_outside_n"]) == 0 and int(z["grid3_grid8x10x8_mv97_n"]) == 97
    for name, (pts, kw) in cases.items():
        v, c, n = R.points_to_voxel(pts, **kw)
        assert len(v) == int(z[name + "_n"]), name
        assert np.array_equal(c, z[name + "_coors"]) and np.array_equal(n, z[name + "_num"]), name
        assert zlib.crc32(np.ascontiguousarray(v).tobytes()) == int(z[name + "_voxels_crc"]), name
        rows = z[name + "_rows"].astype(np.int64)
        filled = rows >= 0
        assert np.array_equal(filled, np.arange(rows.shape[1])[None, :] < n[:, None]), name
        assert np.array_equal(v[filled], np.asarray(pts, np.float32)[rows[filled]]), name


# ---------------------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------------------
def paddle_running_stats(model):
    """torch's BatchNorm modules put the UNBIASED batch variance into running_var; Paddle puts the biased one (stand-in table, L2).  Hooks
    that compute the running update the Paddle way for every BatchNorm of a torch model of the oracle, 0.9 * old + 0.1 * (mean, biased
    variance); settle_running_stats() writes them into the buffers (after the backward pass, which checks the buffers' versions)."""
    def pre(m, inp):
        if m.training:
            x = inp[0].detach()
            axes = [a for a in range(x.dim()) if a != 1]
            rm, rv = getattr(m, "_paddle", None) or (m.running_mean.clone(), m.running_var.clone())
            m._paddle = (0.9 * rm + 0.1 * x.mean(axes), 0.9 * rv + 0.1 * x.var(axes, unbiased=False))

    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.register_forward_pre_hook(pre)


def settle_running_stats(model):
    with torch.no_grad():
        for m in model.modules():
            if getattr(m, "_paddle", None) is not None:
                m.running_mean.copy_(m._paddle[0])
                m.running_var.copy_(m._paddle[1])


@pytest.mark.parametrize("name", MODELS)
def test_checkpoint_names_and_shapes(name):
    """papc_amd/checkpoint.py against the state_dict() the reference's model really has: every recorded key is produced by export_state with
    the recorded shape (Linear [in, out]); what export_state adds is exactly the layers the reference holds in
    plain lists; import_state finds a place for every recorded entry and leaves nothing of the model unfilled"""
    from papc_amd import checkpoint
    model, z = seeded_product(name)
    state, shapes = recorded_state(z)
    out = checkpoint.export_state(model)
    keys = [str(s) for s in z["state_keys"]]
    listed = [str(s) for s in z["list_keys"]]
    assert set(out) == set(keys) | set(listed), sorted(set(out) ^ (set(keys) | set(listed)))
    for k in keys + listed:
        assert tuple(out[k].shape) == shapes[k], (k, out[k].shape, shapes[k])        # (Linear: [in, out], not torch's [out, in])
        assert np.array_equal(out[k], state[k]), k                                   # the round trip returns the value, in the reference's layout
    if name != "ssg_seg":                                                             # (the segmenter's head is two Conv1D)
        assert any(k.endswith(".weight") and len(shapes[k]) == 2 for k in keys)


@pytest.mark.parametrize("name", MODELS)
def test_trainable_parameters_match(name):
    """with reference_quirks=True this project's models train exactly what the reference's parameters() lists (the layers it keeps in plain lists
    are frozen); the other models have no such switch and register everything, as the reference does"""
    from papc_amd import checkpoint
    z = gold("ref_model_" + name)
    kw = dict(reference_quirks=True) if name in ("ssg_clas", "msg_clas", "ssg_seg") else {}
    model = make_product(name, **kw)
    own = sorted(checkpoint._to_reference_name(n, model) for n, p in model.named_parameters() if p.requires_grad)
    assert own == sorted(str(s) for s in z["param_names"])
    frozen = sorted(n for n, p in model.named_parameters() if not p.requires_grad)
    assert frozen == sorted(str(s) for s in z["list_keys"] if not str(s).endswith(("_mean", "_variance")))
    # every trainable parameter of the reference received a gradient from logits.sum(); list-held layers behind an index_points cut did not
    grads = set(str(s) for s in z["grad_names"])
    assert set(str(s) for s in z["param_names"]) <= grads
    if name == "ssg_clas":
        assert not any(g.startswith("sa1.") for g in grads) and any(g.startswith("sa2.") for g in grads) and any(g.startswith("sa3.") for g in grads)
    if name == "ssg_seg":
        assert sorted(set(g.split(".")[0] for g in grads)) == ["bn1", "conv1", "conv2", "fp1"]


def _double_state(model):
    return {k: v.detach().double() for k, v in model.state_dict().items() if not k.endswith("num_batches_tracked")}


def _load(tr_model, P, rename):
    sd = {rename(k): v for k, v in P.items()}
    for k in tr_model.state_dict():
        if k.endswith("num_batches_tracked"):
            sd[k] = tr_model.state_dict()[k]
    tr_model.load_state_dict(sd, strict=True)
    return tr_model.double()


class _MSGClas(nn.Module):
    """PointNet2_MSG_Clas out of the oracle's layers (classify/pointnet2/pointnet2.py: widths and radii from the constructor arguments recorded
    in papc_amd.models, the forward the SSG classifier's)"""

    def __init__(self):
        super().__init__()
        self.sa1 = TR.SetAbstractionMsg(512, [0.1, 0.2, 0.4], [16, 32, 128], 0, [[32, 32, 64], [64, 64, 128], [64, 96, 128]])
        self.sa2 = TR.SetAbstractionMsg(128, [0.2, 0.4, 0.8], [32, 64, 128], 320, [[64, 64, 128], [128, 128, 256], [128, 128, 256]])
        self.sa3 = TR.SetAbstraction(None, None, None, 640 + 3, [256, 512, 1024], True)
        self.fc1, self.bn1, self.drop1 = nn.Linear(1024, 512), nn.BatchNorm1d(512), nn.Dropout(0.0)
        self.fc2, self.bn2, self.drop2 = nn.Linear(512, 256), nn.BatchNorm1d(256), nn.Dropout(0.0)
        self.fc3 = nn.Linear(256, 16)

    forward = TR.SSGClas.forward


class _SSGSeg(nn.Module):
    """PointNet2_SSG_Seg out of the oracle's layers, the forward of torch_cpu_reference.MSGSeg"""

    def __init__(self):
        super().__init__()
        self.num_classes = 16
        self.sa1 = TR.SetAbstraction(512, 0.2, 32, 6, [64, 64, 128], False)
        self.sa2 = TR.SetAbstraction(128, 0.4, 64, 128 + 3, [128, 128, 256], False)
        self.sa3 = TR.SetAbstraction(None, None, None, 256 + 3, [256, 512, 1024], True)
        self.fp3 = TR.FeaturePropagation(1280, [256, 256])
        self.fp2 = TR.FeaturePropagation(384, [256, 128])
        self.fp1 = TR.FeaturePropagation(128 + 16 + 6, [128, 128, 128])
        self.conv1, self.bn1, self.drop1 = nn.Conv1d(128, 128, 1), nn.BatchNorm1d(128), nn.Dropout(0.0)
        self.conv2 = nn.Conv1d(128, 50, 1)

    forward = TR.MSGSeg.forward


def _tr_rename(k):
    return k.replace("mlp_convs", "convs").replace("mlp_bns", "bns")


def _run_tr(name, model, z, lay):
    """-> dict(head_in, train_logits, eval_logits, first / last norm statistics, grad names) of the oracle's torch model in double"""
    P = _double_state(model)
    s = (lay["start1"].astype(np.int64), lay["start2"].astype(np.int64))
    x = torch.from_numpy(np.ascontiguousarray(np.transpose(lay["cloud"], (0, 2, 1))).astype(np.float64))
    if name == "basic_clas":
        names = type(model).reference_names                  # convs.i / bns.i -> the source's mlp_1 / mlp_2 indices, which the oracle's model uses

        def ren(k):
            for own, theirs in names.items():
                if k.startswith(own + "."):
                    return theirs + k[len(own):]
            return k

        tr = _load(TR.BasicClas(num_classes=10), P, ren)
        head, call = tr.fc, lambda: tr(x)
    else:
        tr = _load({"ssg_clas": lambda: TR.SSGClas(), "msg_clas": _MSGClas, "ssg_seg": _SSGSeg}[name](), P, _tr_rename)
        if name == "ssg_seg":
            head, call = tr.conv1, lambda: tr(x, torch.from_numpy(lay["seg_labels"]), s)
        else:
            head, call = tr.fc1, lambda: tr(x, s)
    for m in tr.modules():                                # the recorded forwards draw no dropout mask (see the generator)
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    paddle_running_stats(tr)
    got = {}

    def tap(m, a):
        got.setdefault("head_in", a[0].detach().numpy().copy())

    head.register_forward_pre_hook(tap)
    tr.train()
    logits = call()
    got["train_logits"] = logits.detach().numpy().copy()
    logits.sum().backward()
    got["grads"] = sorted(k for k, p in tr.named_parameters() if p.grad is not None)
    settle_running_stats(tr)
    mods = dict(tr.named_modules())
    for tag in ("first", "last"):
        m = mods[_tr_rename(str(z[tag + "_norm"][0]))]
        got[tag] = (m.running_mean.numpy().copy(), m.running_var.numpy().copy())
    tr.eval()
    for n in z["train_norms_in_eval"]:                    # the reference's eval() never reaches its list-held norms
        mods[_tr_rename(str(n))].train()
    with torch.no_grad():
        got["eval_logits"] = call().numpy().copy()
    return got


@pytest.mark.parametrize("name", ["ssg_clas", "msg_clas", "ssg_seg", "basic_clas"])
def test_oracle_models_float64(name, lay):
    """oracle/torch_cpu_reference.py's models (and the two it does not spell out, composed of its layers) in double, with the seeded weights
    loaded through checkpoint.import_state into this project's model and from there by name: head input, logits, running statistics and the
    eval-mode logits against the reference's own execution at 1e-9; the parameters that hold a gradient are the recorded ones"""
    model, z = seeded_product(name)
    got = _run_tr(name, model, z, lay)
    cut = (lambda a: a[..., ::SEG_STRIDE]) if name == "ssg_seg" else (lambda a: a)
    cutl = (lambda a: a[:, ::SEG_STRIDE]) if name == "ssg_seg" else (lambda a: a)
    close64(cut(got["head_in"]), z["head_in"], name + " head input")
    close64(cutl(got["train_logits"]), z["train_logits"], name + " train logits")
    for tag in ("first", "last"):
        close64(got[tag][0], z[tag + "_mean"], "%s %s running mean" % (name, z[tag + "_norm"][0]))
        close64(got[tag][1], z[tag + "_var"], "%s %s running variance" % (name, z[tag + "_norm"][0]))
    close64(cutl(got["eval_logits"]), z["eval_logits"], name + " eval logits")
    if name != "basic_clas":
        assert got["grads"] == sorted(_tr_rename(str(s)) for s in z["grad_names"])


def test_pointnet_clas_twin_float64(lay):
    from tests import pointnet_ref
    model, z = seeded_product("pointnet_clas")
    x = torch.from_numpy(np.ascontiguousarray(np.transpose(lay["cloud"], (0, 2, 1))).astype(np.float64))
    logits = pointnet_ref.pointnet_clas(_double_state(model), x, train=True, drop_p=0.0)
    close64(logits.detach().numpy(), z["train_logits"], "pointnet_clas train logits (tests/pointnet_ref.py)")


def test_kdnet_twin_float64():
    from tests import kdnet_ref
    model, z = seeded_product("kdnet")
    kd = gold("kdtree_n1024")
    sels = [kd["split_%d" % i].astype(np.int64) for i in range(10)]
    P = _double_state(model)
    x = torch.from_numpy(z["points"].astype(np.float64))
    close64(kdnet_ref.kdnet(P, x, sels).detach().numpy(), z["eval_logits"], "kdnet logits (tests/kdnet_ref.py)")
    assert np.array_equal(z["eval_logits"], z["train_logits"])                       # no norm, no dropout: train == eval
    ident = dict(P)
    ident["fc.weight"], ident["fc.bias"] = torch.eye(128, dtype=torch.float64), torch.zeros(128, dtype=torch.float64)
    close64(kdnet_ref.kdnet(ident, x, sels).detach().numpy(), z["head_in"], "kdnet head input")


def test_voxnet_twin_float64():
    from tests import voxnet_ref
    model, z = seeded_product("voxnet")
    P = _double_state(model)
    x = torch.from_numpy(np.unpackbits(z["grid_bits"]).reshape(3, 1, 32, 32, 32).astype(np.float64))
    logits, aux = voxnet_ref.literal(P, x)
    close64(aux["flat"].detach().numpy(), z["head_in"], "voxnet head input")
    close64(logits.detach().numpy(), z["train_logits"], "voxnet train logits")
    rm, rv = 0.1 * aux["mean"].detach(), 0.9 + 0.1 * aux["var"].detach()          # 0.9 * (0, 1) + 0.1 * (batch mean, biased batch variance)
    close64(rm.numpy(), z["first_mean"], "voxnet running mean")
    close64(rv.numpy(), z["first_var"], "voxnet running variance")
    ev, _ = voxnet_ref.literal(P, x, stats=(rm, rv))
    close64(ev.detach().numpy(), z["eval_logits"], "voxnet eval logits")
