"""Regenerates tests/golden/ref_*.npz: what the REFERENCE'S OWN model code computes when it is executed on the paddle stand-in
(oracle/paddle_standin, torch-CPU underneath).  Needs a checkout of the reference; only arrays, names and seeds are committed.

    python tests/golden/make_reference_golden.py /path/to/reference          (the directory that holds PAPC/)

The reference is reached only through that path: ``PAPC.models.layers`` / ``.classify`` / ``.segment`` are imported from it unmodified
(recording wrappers are put around its sampling functions from outside), and its voxeliser header is compiled through the ten-line wrapper
oracle/ref_voxel_wrapper.cc into oracle/_ref/ (kept out of git).  Running it twice gives byte-identical files (fixed zip timestamps).

Files (float values of the float64-mode run are float64, inputs float32, indices int16, no weights: tests.util.reference_weight is the rule):
  ref_layers.npz   the input clouds and square_distance, farthest_point_sample, query_ball_point, each in float32 mode (``*_32``) and
                   float64 mode (``*_64``; indices, identical in both, are stored once)
  ref_group.npz    sample_and_group, sample_and_group_all and one PointNetSetAbstraction layer, in both modes
  ref_fp.npz       PointNetFeaturePropagation.forward (S = 64 and the S == 1 branch) with its sorted distances and argsort-of-sorted indices
  ref_voxel.npz    points_to_voxel<float, 3> on the tests/detect_cases.py inputs
  ref_model_<name>.npz   per model: state_dict keys / shapes, parameters() names, list-held layer names, sampling indices of a train-mode forward,
                   the tensor entering the head, its logits, running statistics of the first and last norm, eval-mode logits, gradient holders

INPUT CONDITIONS (asserted on the float64 run: ``check_recorded``, ``same_indices``, ``pyramid_violations``).  Every squared distance is a relative 1e-5 away from r^2, every FPS winner
beats the runner-up by a relative 1e-5 (the lattice case is exact and exempt), the first neighbour distances of every FP query are
separated by a relative 1e-5, and the float32-mode run gives the same indices.  Under these any correct fp32 evaluation order yields the
same indices.  At B = 2, N = 1024, npoint = 512 a plain random cloud violates them about a dozen times (1280 FPS iterations, ~5 million
centroid-point pairs over the models' radii; the first seed as drawn: 11 points), so a clean draw has a probability near e^-11 and walking
seeds does not end; each seed of SEEDS is therefore REPAIRED: the point behind a violation is moved by about 1e-4 (seeded), until a pass finds none.  The
stored cloud is the repaired one.
"""
import io
import os
import subprocess
import sys
import sysconfig
import zipfile
import zlib

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.paddle_standin import on_path          # noqa: E402
from tests.util import fps_lattice, reference_weight   # noqa: E402

SEEDS = (20250101, 20250102, 20250103)
WEIGHT_SEED = 7
REL = 1e-5
B, N = 2, 1024
HALF = 0.28                      # clouds live in [-HALF, HALF]^3: every squared distance < 1, the FPS running distance starts at ones
# every (level, radius) the recorded models and layer cases query: level 0 = the cloud -> 512 centroids, level 1 = those 512 -> 128
RADII = {0: (0.05, 0.1, 0.2, 0.4), 1: (0.2, 0.4, 0.8)}
FP_S = slice(300, 364)           # the standalone FP case: the support points of the cloud
FP_MIN_D2 = 4e-3                 # ... and its 256 query points: the first ones whose nearest support point is at least this squared distance away.
# The reference's own formula 1 / (d + 1e-8) over d = -2 a.b + |a|^2 + |b|^2 loses the small distances to cancellation in float32 (absolute
# error ~3 * 2^-24 * (|a|^2 + |b|^2) ~ 6e-8, i.e. 4e-4 of d = 1.5e-4): on the first 256 points of the cloud the reference's OWN float32-mode
# output is 1.1e-3 elementwise from its float64 run, over the project's per-layer bar before any kernel has run.  With d >= 4e-3 the weights
# move by 1.5e-5; fp_cases asserts that the reference's float32 mode then stays within a third of the elementwise bar.  (The near regime,
# d = 0 included, is what the segmentation model's fp1 / fp2 levels run on, at the model-level bar.)
FP_OWN_ELEMENTWISE = 1e-3 / 3
SEG_STRIDE = 32                  # the segmenter's per-point tensors are stored for every 32nd point


# ---------------------------------------------------------------------------------------------------------------------------------------
# deterministic .npz
# ---------------------------------------------------------------------------------------------------------------------------------------
def save_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[k])
            np.lib.format.write_array(buf, np.ascontiguousarray(a) if a.ndim else a, allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    assert size < 240 * 1024, (path, size)
    print("%s: %d bytes" % (os.path.basename(path), size))


def names_array(names):
    return np.array(list(names), dtype="U") if len(names) else np.zeros((0,), "U1")


def shapes_array(shapes):
    out = -np.ones((len(shapes), 5), np.int32)
    for i, s in enumerate(shapes):
        out[i, :len(s)] = s
    return out


def idx16(a):
    a = np.asarray(a)
    assert a.min() >= 0 and a.max() < 2 ** 15 and np.all(a == np.round(a))
    return a.astype(np.int16)


def crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the input conditions, in float64 numpy (our own arithmetic: it only JUDGES inputs; every recorded index comes from the reference's code)
# ---------------------------------------------------------------------------------------------------------------------------------------
def fps_f64(xyz, npoint, start):
    """-> (indices [B, npoint], list of (cloud, runner-up point) whose margin is below REL)"""
    xyz = np.asarray(xyz, np.float64)
    nb, n, _ = xyz.shape
    dist = np.ones((nb, n))
    far = np.asarray(start, np.int64).copy()
    out = np.zeros((nb, npoint), np.int64)
    bad = []
    ar = np.arange(nb)
    for i in range(npoint):
        out[:, i] = far
        d = ((xyz - xyz[ar, far][:, None, :]) ** 2).sum(-1)
        dist = np.minimum(dist, d)
        far = dist.argmax(-1)
        if i + 1 < npoint:
            top = dist[ar, far]
            rest = dist.copy()
            rest[ar, far] = -1.0
            second = rest.argmax(-1)
            for b in range(nb):
                if top[b] - rest[b, second[b]] < REL * top[b]:
                    bad.append((b, int(second[b])))
    return out, bad


def sqd_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)


def ball_bad(xyz, new_xyz, radius):
    """(cloud, point) of every pair whose squared distance lies within REL * r^2 of r^2"""
    d = sqd_f64(new_xyz, xyz)
    r2 = float(radius) ** 2
    b, _, j = np.nonzero(np.abs(d - r2) < REL * r2)
    return list(zip(b.tolist(), j.tolist()))


def nn_bad(xyz1, xyz2):
    """(cloud, query) whose four smallest distances are not separated by REL of the larger one"""
    d = np.sort(sqd_f64(xyz1, xyz2), -1)[:, :, :4]
    gap = d[:, :, 1:] - d[:, :, :-1]
    b, q = np.nonzero((gap < REL * d[:, :, 1:]).any(-1))
    return list(zip(b.tolist(), q.tolist()))


def pyramid_violations(cloud, s1, s2):
    """every violation of the input conditions over the two-level sampling pyramid the models run on ``cloud`` [B, N, 3] -> list of
    (cloud index, index of the point to move)"""
    i1, bad = fps_f64(cloud, 512, s1)
    ar = np.arange(cloud.shape[0])[:, None]
    l1 = cloud[ar, i1]
    i2, bad2 = fps_f64(l1, 128, s2)
    bad += [(b, int(i1[b, j])) for b, j in bad2]
    l2 = l1[ar, i2]
    for r in RADII[0]:
        bad += ball_bad(cloud, l1, r)
    for r in RADII[1]:
        bad += [(b, int(i1[b, j])) for b, j in ball_bad(l1, l2, r)]
    bad += nn_bad(cloud, l1)                                          # fp1: queries are the cloud's points
    bad += [(b, int(i1[b, q])) for b, q in nn_bad(l1, l2)]            # fp2
    bad += nn_bad(cloud, cloud[:, FP_S])                              # the standalone FP case (its queries are points of the cloud)
    return bad


def make_cloud(seed):
    """a float32 cloud [B, N, 3] in the cube and start indices that meet the conditions on the models' pyramid, by repair (module docstring)"""
    rng = np.random.default_rng(seed)
    cloud = rng.uniform(-HALF, HALF, (B, N, 3)).astype(np.float32)
    s1 = rng.integers(0, N, B)
    s2 = rng.integers(0, 512, B)
    for rounds in range(400):
        bad = sorted(set(pyramid_violations(cloud, s1, s2)))
        if rounds == 0:
            print("seed %d: %d points behind violations of the input conditions as drawn" % (seed, len(bad)))
        if not bad:
            print("seed %d: input conditions hold after %d repair rounds" % (seed, rounds))
            return cloud, s1, s2
        for b, j in bad:
            step = rng.normal(size=3) * 1e-4
            cloud[b, j] = np.clip(cloud[b, j].astype(np.float64) + step, -HALF, HALF).astype(np.float32)
    return None


# ---------------------------------------------------------------------------------------------------------------------------------------
# running the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
class Recorder:
    """wrappers around the reference's farthest_point_sample / query_ball_point and the stand-in's sort / argsort: what they returned, in call order"""

    def __init__(self, paddle, L):
        self.paddle, self.L = paddle, L
        self.fps, self.ball, self.sorted, self.argsorted = [], [], [], []

    def __enter__(self):
        L, p = self.L, self.paddle
        self.saved = (L.farthest_point_sample, L.query_ball_point, p.sort, p.argsort)
        f_fps, f_ball, f_sort, f_argsort = self.saved

        def fps(xyz, npoint):
            out = f_fps(xyz, npoint)
            self.fps.append((xyz.numpy().copy(), out.numpy().copy()))
            return out

        def ball(radius, nsample, xyz, new_xyz):
            out = f_ball(radius, nsample, xyz, new_xyz)
            self.ball.append((radius, nsample, xyz.numpy().copy(), new_xyz.numpy().copy(), out.numpy().copy()))
            return out

        def sort(x, axis=-1, descending=False):
            out = f_sort(x, axis, descending)
            self.sorted.append(out.numpy().copy())
            return out

        def argsort(x, axis=-1, descending=False):
            out = f_argsort(x, axis, descending)
            self.argsorted.append(out.numpy().copy())
            return out

        L.farthest_point_sample, L.query_ball_point, p.sort, p.argsort = fps, ball, sort, argsort
        return self

    def __exit__(self, *exc):
        L, p = self.L, self.paddle
        L.farthest_point_sample, L.query_ball_point, p.sort, p.argsort = self.saved


def held_layers(model, nn):
    """[(name, layer)] of every weight-carrying layer, registered or kept in a plain list, named as this project names them
    (``sa1.mlp_convs.0``, ``sa1.conv_blocks.1.2``), in the order a forward visits the containers"""
    out = []

    def visit(prefix, obj):
        if isinstance(obj, (list, tuple)):
            for i, v in enumerate(obj):
                visit("%s.%d" % (prefix, i), v)
        elif isinstance(obj, nn.Layer):
            if obj._parameters:
                out.append((prefix, obj))
            for n, sub in obj._sub_layers.items():
                visit((prefix + "." if prefix else "") + n, sub)
            for n, v in vars(obj).items():
                if isinstance(v, (list, tuple)) and v and not n.startswith("_"):
                    visit((prefix + "." if prefix else "") + n, v)

    visit("", model)
    return out


def seed_weights(model, nn):
    """reference_weight into every trainable tensor; returns (registered names, list-held names -> shape)"""
    registered = set(model.state_dict().keys())
    listed = {}
    for lname, layer in held_layers(model, nn):
        for pname, p in layer._parameters.items():
            name = lname + "." + pname
            with torch.no_grad():
                p.copy_(torch.from_numpy(reference_weight(name, tuple(p.shape), WEIGHT_SEED)).to(p.dtype))
            if name not in registered:
                listed[name] = tuple(p.shape)
        for bname, b in layer._buffers.items():
            if lname + "." + bname not in registered:
                listed[lname + "." + bname] = tuple(b.shape)
    return listed


def run_model(paddle, nn, L, make, inputs, head, starts, seg=False):
    """one train-mode forward + backward and one eval-mode forward of a reference model in float64 mode -> dict of arrays"""
    paddle.set_float("float64")
    model = make()
    listed = seed_weights(model, nn)
    out = {}
    sd = model.state_dict()
    out["state_keys"] = names_array(sd.keys())
    out["state_shapes"] = shapes_array([tuple(v.shape) for v in sd.values()])
    pnames = [n for n, _ in model.named_parameters()]
    assert len(pnames) == len(model.parameters())
    out["param_names"] = names_array(pnames)
    out["list_keys"] = names_array(listed.keys())
    out["list_shapes"] = shapes_array(list(listed.values()))
    held = held_layers(model, nn)
    # the recorded forwards draw no dropout mask (p = 0 on every Dropout): the product draws its masks on the device and takes none from
    # outside, so a masked train forward could not be compared; Dropout's train rule is held by the stand-in's known-answer case
    for _, l in model.named_sublayers(include_self=True):
        if isinstance(l, nn.Dropout):
            l.p = 0.0
    norm_order, head_in = [], []
    for name, l in held:
        if isinstance(l, nn.BatchNorm):
            l.register_forward_post_hook(lambda layer, a, o, name=name: norm_order.append(name))
    getattr(model, head).register_forward_pre_hook(lambda layer, a: head_in.append(a[0].numpy().copy()))
    f64 = lambda v: np.asarray(v, np.float64) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v
    x = [f64(v) for v in inputs] if isinstance(inputs, list) else f64(inputs)
    model.train()
    paddle.RANDINT_QUEUE[:] = [np.asarray(s) for s in starts]
    with Recorder(paddle, L) as rec:
        logits = model(x)
    assert not paddle.RANDINT_QUEUE
    tl = logits.numpy().copy()
    out["train_logits"] = tl[:, ::SEG_STRIDE] if seg else tl
    logits.sum().backward()
    named = dict(model.named_parameters())
    for lname, layer in held:
        for pname, p in layer._parameters.items():
            named.setdefault(lname + "." + pname, p)
    out["grad_names"] = names_array([n for n, p in named.items() if p.grad is not None])
    for i, (_, idx) in enumerate(rec.fps):
        out["fps_%d" % i] = idx16(idx)
    for i, (radius, nsample, xyz, new_xyz, idx) in enumerate(rec.ball):
        out["ball_%d_rows" % i] = idx16(idx[:, ::4])
        out["ball_%d_crc" % i] = crc(idx.astype(np.int16))
        out["ball_%d_meta" % i] = np.array([radius, nsample, xyz.shape[1], new_xyz.shape[1]], np.float64)
    h = head_in[0]
    out["head_in"] = h[..., ::SEG_STRIDE] if seg else h
    dicts = dict(held)
    order = list(dict.fromkeys(norm_order))
    out["norm_order"] = names_array(order)
    for tag, name in (("first", order[0]), ("last", order[-1])) if order else ():
        out[tag + "_norm"] = names_array([name])
        out[tag + "_mean"] = dicts[name]._mean.numpy().copy()
        out[tag + "_var"] = dicts[name]._variance.numpy().copy()
    model.eval()
    paddle.RANDINT_QUEUE[:] = [np.asarray(s) for s in starts]
    with Recorder(paddle, L) as rec2:
        ev = model(x).numpy()
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(rec.fps, rec2.fps))
    out["eval_logits"] = ev[:, ::SEG_STRIDE] if seg else ev
    out["train_norms_in_eval"] = names_array([n for n, l in held if isinstance(l, nn.BatchNorm) and l.training])
    out["weight_seed"] = np.int64(WEIGHT_SEED)
    # what the reference ITSELF loses in float32 (Paddle's own precision): the same two forwards in float32 mode, as (max-norm, elementwise on
    # entries >= 1e-3 of the maximum) deviations from the float64 run.  The pin tests never hold fp32 kernels elementwise tighter than 3 x this.
    h32, ev32 = float32_run(paddle, nn, L, make, inputs, head, starts)
    for key, a32, ref in (("head_in", h32, h), ("eval_logits", ev32, ev)):
        scale = np.abs(ref).max()
        big = np.abs(ref) >= 1e-3 * scale
        dev = np.abs(a32.astype(np.float64) - ref)
        out["own32_" + key] = np.array([dev.max() / scale, (dev[big] / np.abs(ref)[big]).max()])
        print("    float32 mode vs float64, %s: %.2e of max, %.2e elementwise" % (key, out["own32_" + key][0], out["own32_" + key][1]))
    return out, rec


def float32_run(paddle, nn, L, make, inputs, head, starts):
    """(head input, eval-mode logits) of the same model, weights and inputs in float32 mode"""
    paddle.set_float("float32")
    try:
        model = make()
        seed_weights(model, nn)
        for _, l in model.named_sublayers(include_self=True):
            if isinstance(l, nn.Dropout):
                l.p = 0.0
        head_in = []
        getattr(model, head).register_forward_pre_hook(lambda layer, a: head_in.append(a[0].numpy().copy()))
        model.train()
        paddle.RANDINT_QUEUE[:] = [np.asarray(s) for s in starts]
        model(inputs)
        model.eval()
        paddle.RANDINT_QUEUE[:] = [np.asarray(s) for s in starts]
        ev = model(inputs).numpy()
        assert head_in[0].dtype == np.float32 and ev.dtype == np.float32
        return head_in[0], ev
    finally:
        paddle.set_float("float64")


def layer_cases(paddle, nn, L, mode, cloud, s1, lat, slat, queries):
    """the layer functions in one float mode -> ({key: array}, Recorder)"""
    paddle.set_float(mode)
    dt = np.float32 if mode == "float32" else np.float64
    t = lambda a: paddle.to_tensor(np.asarray(a, dt))
    o = {}
    with Recorder(paddle, L) as rec:
        o["sqdist"] = L.square_distance(t(cloud[:, :64]), t(cloud[:, 100:200])).numpy()
        paddle.RANDINT_QUEUE[:] = [s1]
        o["fps_cloud"] = idx16(L.farthest_point_sample(t(cloud), 128).numpy())
        paddle.RANDINT_QUEUE[:] = [slat]
        o["fps_lattice"] = idx16(L.farthest_point_sample(t(lat), 64).numpy())
        centres = cloud[np.arange(B)[:, None], o["fps_cloud"].astype(np.int64)]
        o["ball_r02"] = idx16(L.query_ball_point(0.2, 32, t(cloud), t(centres)).numpy())
        o["ball_r005"] = idx16(L.query_ball_point(0.05, 16, t(cloud), t(queries)).numpy())      # queries beside the cloud: some hit nothing
        feats = np.transpose(cloud, (0, 2, 1))[:, ::-1, :] * 2.0 + 0.25                           # any [B, 3, N] features
        paddle.RANDINT_QUEUE[:] = [s1]
        new_xyz, new_points, grouped_xyz, fps_idx = L.sample_and_group(32, 0.2, 16, t(cloud), t(np.transpose(feats, (0, 2, 1))), returnfps=True)
        o["sg_new_xyz"], o["sg_new_points"], o["sg_fps"] = new_xyz.numpy(), new_points.numpy(), idx16(fps_idx.numpy())
        a, b = L.sample_and_group_all(t(cloud[:, :128]), t(np.transpose(feats, (0, 2, 1))[:, :128]))
        o["sga_new_xyz"], o["sga_new_points"] = a.numpy(), b.numpy()
        sa = L.PointNetSetAbstraction(32, 0.2, 16, 3 + 3, [16, 32], False)
        for lname, layer in held_layers(sa, nn):
            for pname, p in layer._parameters.items():
                with torch.no_grad():
                    p.copy_(torch.from_numpy(reference_weight("sa." + lname + "." + pname, tuple(p.shape), WEIGHT_SEED)).to(p.dtype))
        paddle.RANDINT_QUEUE[:] = [s1]
        a, b = sa(t(np.transpose(cloud, (0, 2, 1))), t(feats))
        o["sa_new_xyz"], o["sa_new_points"] = a.numpy(), b.numpy()
        o["sa_mean0"], o["sa_var0"] = sa.mlp_bns[0]._mean.numpy().copy(), sa.mlp_bns[0]._variance.numpy().copy()
        assert sa.parameters() == [] and b.grad_fn is not None
    return o, rec


def fp_cases(paddle, nn, L, cloud):
    paddle.set_float("float64")
    t = lambda a: paddle.to_tensor(np.asarray(a, np.float64))
    o = {}
    rng = np.random.default_rng(WEIGHT_SEED + 1)
    near = sqd_f64(cloud, cloud[:, FP_S]).min(-1)
    qidx = np.stack([np.nonzero(near[b] >= FP_MIN_D2)[0][:256] for b in range(B)])
    assert qidx.shape == (B, 256)
    o["fp_query_idx"] = idx16(qidx)
    queries = cloud[np.arange(B)[:, None], qidx]
    xyz1 = np.transpose(queries, (0, 2, 1))
    xyz2 = np.transpose(cloud[:, FP_S], (0, 2, 1))
    p1 = rng.normal(size=(B, 6, 256)).astype(np.float32)
    p2 = rng.normal(size=(B, 16, 64)).astype(np.float32)
    o.update(fp_points1=p1, fp_points2=p2)
    for tag, x2, q2 in (("s64", xyz2, p2), ("s1", xyz2[:, :, :1], p2[:, :, :1])):
        fp = L.PointNetFeaturePropagation(6 + 16, [32, 16])
        for lname, layer in held_layers(fp, nn):
            for pname, p in layer._parameters.items():
                with torch.no_grad():
                    p.copy_(torch.from_numpy(reference_weight("fp." + lname + "." + pname, tuple(p.shape), WEIGHT_SEED)).to(p.dtype))
        with Recorder(paddle, L) as rec:
            out = fp(t(xyz1), t(x2), t(p1), t(q2))
        o["fp_%s_out" % tag] = out.numpy()
        o["fp_%s_mean0" % tag], o["fp_%s_var0" % tag] = fp.mlp_bns[0]._mean.numpy().copy(), fp.mlp_bns[0]._variance.numpy().copy()
        if tag == "s64":
            assert len(rec.sorted) == 1 and len(rec.argsorted) == 1
            o["fp_s64_dist3"] = rec.sorted[0][:, :, :3]
            o["fp_s64_idx3"] = idx16(rec.argsorted[0][:, :, :3])
            assert not nn_bad(queries, cloud[:, FP_S]), "FP case: neighbour distances too close"
        else:
            assert not rec.sorted and not rec.argsorted          # the S == 1 branch sorts nothing
    paddle.set_float("float32")
    with Recorder(paddle, L) as rec:
        fp = L.PointNetFeaturePropagation(6 + 16, [32, 16])
        for lname, layer in held_layers(fp, nn):
            for pname, p in layer._parameters.items():
                with torch.no_grad():
                    p.copy_(torch.from_numpy(reference_weight("fp." + lname + "." + pname, tuple(p.shape), WEIGHT_SEED)).to(p.dtype))
        out = fp(paddle.to_tensor(xyz1.astype(np.float32)), paddle.to_tensor(xyz2.astype(np.float32)), paddle.to_tensor(p1), paddle.to_tensor(p2))
    o["fp_s64_out_32"] = out.numpy()
    assert o["fp_s64_out_32"].dtype == np.float32
    ref = o["fp_s64_out"]
    big = np.abs(ref) >= 1e-3 * np.abs(ref).max()
    own = float((np.abs(o["fp_s64_out_32"] - ref)[big] / np.abs(ref)[big]).max())
    print("FP case: the reference's float32 mode is %.2e elementwise from its float64 run" % own)
    assert own <= FP_OWN_ELEMENTWISE, own
    assert np.array_equal(idx16(rec.argsorted[0][:, :, :3]), o["fp_s64_idx3"])
    o["fp_s64_dist3_32"] = rec.sorted[0][:, :, :3]
    return o


def check_recorded(rec, exempt_lattice_calls=()):
    """the input conditions on every sampling call a run made (float64 run)"""
    for i, (xyz, idx) in enumerate(rec.fps):
        if i in exempt_lattice_calls:
            continue
        mine, bad = fps_f64(xyz, idx.shape[1], idx[:, 0])
        assert np.array_equal(mine, idx.astype(np.int64)) and not bad, "FPS call %d: winner margin below 1e-5" % i
    for radius, nsample, xyz, new_xyz, idx in rec.ball:
        assert not ball_bad(xyz, new_xyz, radius), "ball query r = %g: a squared distance within 1e-5 of r^2" % radius


def same_indices(r32, r64):
    assert len(r32.fps) == len(r64.fps) and len(r32.ball) == len(r64.ball)
    for a, b in zip(r32.fps, r64.fps):
        assert np.array_equal(a[1], b[1]), "float32 and float64 mode disagree on FPS indices"
    for a, b in zip(r32.ball, r64.ball):
        assert np.array_equal(a[4], b[4]), "float32 and float64 mode disagree on ball-query indices"


# ---------------------------------------------------------------------------------------------------------------------------------------
# voxeliser
# ---------------------------------------------------------------------------------------------------------------------------------------
def build_voxel_wrapper(ref):
    """oracle/ref_voxel_wrapper.cc + the reference's point_cloud_ops.h -> oracle/_ref/ref_voxel*.so"""
    import pybind11
    cc_dir = os.path.join(ref, "PAPC", "models", "detect", "pointpillars", "libs", "ops", "cc")
    out_dir = os.path.join(ROOT, "oracle", "_ref")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "ref_voxel" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-std=c++14", "-I" + cc_dir, "-I" + pybind11.get_include(),
                           "-I" + sysconfig.get_paths()["include"], os.path.join(ROOT, "oracle", "ref_voxel_wrapper.cc"), "-o", so])
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_voxel", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def voxel_cases(mod):
    """the reference's compiled loop on tests/detect_cases.py's inputs, driven the way its Python caller does (point_cloud_ops.py:106-166:
    reversed grid shape, -1 filled cell table, zero filled outputs); reverse_index only, which is all the C++ implements"""
    from tests import detect_cases as D
    cases = {}
    for name, (pts, kw) in D.voxel_small_cases().items():
        cases["small_" + name] = (pts, kw)
    cases["lattice"] = (D.lattice_points(), dict(D.LATTICE_KW))
    for grid, g in D.GRIDS3.items():
        for mv in D.GRID3_MAX_VOXELS:
            cases["grid3_%s_mv%d" % (grid, mv)] = (D.grid3_points(3), dict(max_points=D.GRID3_MAX_POINTS, reverse_index=True, max_voxels=mv, **g))
    out = {"case_names": names_array(cases.keys())}
    for name, (pts, kw) in cases.items():
        assert kw["reverse_index"]
        pts = np.ascontiguousarray(pts, np.float32)
        vs, cr = np.asarray(kw["voxel_size"], np.float32), np.asarray(kw["coors_range"], np.float32)
        grid = tuple(np.round((cr[3:] - cr[:3]) / vs).astype(np.int32).tolist())[::-1]
        voxels = np.zeros((kw["max_voxels"], kw["max_points"], pts.shape[1]), np.float32)
        coors = np.zeros((kw["max_voxels"], 3), np.int32)
        num = np.zeros((kw["max_voxels"],), np.int32)
        table = -np.ones(grid, np.int32)
        n = mod.points_to_voxel(pts, voxels, coors, num, table, [float(v) for v in vs], [float(v) for v in cr], kw["max_points"], kw["max_voxels"])
        out[name + "_n"] = np.int32(n)
        out[name + "_coors"] = coors[:n].astype(np.int16)
        out[name + "_num"] = num[:n].astype(np.int16)
        out[name + "_voxels_crc"] = crc(voxels[:n])
        # the points' own row numbers instead of their floats: which input row sits in slot (voxel, t), -1 = empty (exact, and small)
        key = {p.tobytes(): i for i, p in reversed(list(enumerate(pts)))}
        rows = -np.ones((n, kw["max_points"]), np.int32)
        for v in range(n):
            for t_ in range(num[v]):
                rows[v, t_] = key[voxels[v, t_].tobytes()]
        out[name + "_rows"] = rows.astype(np.int16 if len(pts) < 2 ** 15 else np.int32)
    return out


def main():
    ref = os.path.abspath(sys.argv[1])
    gold = HERE
    chosen = None
    for seed in SEEDS:
        made = make_cloud(seed)
        if made is not None:
            chosen = seed
            break
    assert chosen is not None, "no seed of SEEDS could be repaired to meet the input conditions"
    cloud, s1, s2 = made
    rng = np.random.default_rng(chosen + 1)
    queries = rng.uniform(-HALF, HALF, (B, 48, 3)).astype(np.float32)
    while ball_bad(cloud, queries, 0.05):
        queries = rng.uniform(-HALF, HALF, (B, 48, 3)).astype(np.float32)
    assert (sqd_f64(queries, cloud).min(-1) > 0.05 ** 2).any(), "no query without a hit"
    lat = fps_lattice(B, 5)[:, :512]
    slat = np.array([3, 100])
    labels = np.array([[3], [11]], np.int64)
    kd = np.load(os.path.join(gold, "kdtree_n1024.npz"))
    kd_points = np.stack([kd["leaf_points"].T, (kd["leaf_points"] * np.float32(0.75) + np.float32(0.125)).T]).astype(np.float32)
    kd_splits = [kd["split_%d" % i].astype(np.int64) for i in range(10)]
    grid_bits = np.packbits(np.random.default_rng(chosen + 2).random((3, 1, 32, 32, 32)) < 0.08)
    grid = np.unpackbits(grid_bits).reshape(3, 1, 32, 32, 32).astype(np.float32)
    planar = np.ascontiguousarray(np.transpose(cloud, (0, 2, 1)))

    with on_path(ref):
        import paddle
        import paddle.nn as nn
        import PAPC.models.layers.pointnet2_basic_layers as L
        import PAPC.models.classify as C
        import PAPC.models.segment as S
        paddle.TIE_RULE = "all"

        o32, r32 = layer_cases(paddle, nn, L, "float32", cloud, s1, lat, slat, queries)
        o64, r64 = layer_cases(paddle, nn, L, "float64", cloud, s1, lat, slat, queries)
        same_indices(r32, r64)
        check_recorded(r64, exempt_lattice_calls=(1,))
        # the float32-mode distance rows must be the canonical chain of oracle/papc_oracle.c: torch's K = 3 matmul is, on
        # this host; on a host where it is not, generate elsewhere rather than record another rounding
        from oracle import reference_np
        canon = reference_np.square_distance(cloud[:, :64], cloud[:, 100:200])
        assert np.array_equal(canon.view(np.int32), o32["sqdist"].view(np.int32)), "torch's matmul on this host is not the canonical fp32 chain"
        lay = dict(seed=np.int64(chosen), cloud=cloud, start1=idx16(s1), start2=idx16(s2), lattice_seed=np.int64(5), lattice_n=np.int64(512),
                   lattice_start=idx16(slat), queries=queries, seg_labels=labels, weight_seed=np.int64(WEIGHT_SEED))
        for k in o64:
            if o64[k].dtype == np.int16:
                assert np.array_equal(o32[k], o64[k]), k
                lay[k] = o64[k]
            else:
                assert o32[k].dtype == np.float32 and o64[k].dtype == np.float64, (k, o32[k].dtype, o64[k].dtype)
                lay[k + "_32"], lay[k + "_64"] = o32[k], o64[k]
        grp = {k: lay.pop(k) for k in list(lay) if k.startswith(("sg_", "sga_", "sa_"))}
        save_npz(os.path.join(gold, "ref_layers.npz"), lay)
        save_npz(os.path.join(gold, "ref_group.npz"), grp)
        save_npz(os.path.join(gold, "ref_fp.npz"), fp_cases(paddle, nn, L, cloud))

        models = {
            "ssg_clas": (lambda: C.PointNet2_SSG_Clas(), planar, "fc1", [s1, s2], False),
            "msg_clas": (lambda: C.PointNet2_MSG_Clas(), planar, "fc1", [s1, s2], False),
            "ssg_seg": (lambda: S.PointNet2_SSG_Seg(), [planar, labels], "conv1", [s1, s2], True),
            "basic_clas": (lambda: C.PointNet_Basic_Clas(), planar, "fc", [], False),
            "pointnet_clas": (lambda: C.PointNet_Clas(max_point=N), planar, "fc", [], False),
            "kdnet": (lambda: C.KDNet(), [kd_points, kd_splits], "fc", [], False),
            "voxnet": (lambda: C.VoxNet(), grid, "head", [], False),
        }
        for name, (make, inputs, head, starts, seg) in models.items():
            out, rec = run_model(paddle, nn, L, make, inputs, head, starts, seg)
            check_recorded(rec)
            if rec.fps:                                 # the float32-mode pyramid on the same inputs: same indices
                paddle.set_float("float32")
                with Recorder(paddle, L) as rec32:
                    for (xyz, idx) in rec.fps:
                        paddle.RANDINT_QUEUE[:] = [idx[:, 0].astype(np.int64)]
                        L.farthest_point_sample(paddle.to_tensor(xyz.astype(np.float32)), idx.shape[1])
                    for (radius, nsample, xyz, new_xyz, idx) in rec.ball:
                        L.query_ball_point(radius, nsample, paddle.to_tensor(xyz.astype(np.float32)), paddle.to_tensor(new_xyz.astype(np.float32)))
                same_indices(rec32, rec)
            if name == "kdnet":
                out["points"] = kd_points
            if name == "voxnet":
                out["grid_bits"] = grid_bits
            save_npz(os.path.join(gold, "ref_model_%s.npz" % name), out)

    save_npz(os.path.join(gold, "ref_voxel.npz"), voxel_cases(build_voxel_wrapper(ref)))


if __name__ == "__main__":
    main()
