"""GPU parity of the MFMA MLP stack (forward vs the oracle, backward vs a torch float64 autograd reference)."""
import numpy as np
import pytest
import torch

from oracle import reference_np as R
from papc_amd import _lib
from papc_amd import functional as F
from papc_amd.layers import PointNetSetAbstraction, PointNetSetAbstractionMsg
from papc_amd.mlp import StackSpec, shared_mlp_max
from papc_amd.stack import SharedMLPStack
from papc_amd.synthetic import make_clouds, make_start_idx
from tests import torch_ref
from tests.util import assert_close, seeded_weights

pytestmark = pytest.mark.gpu

REL = 1e-5   # north-star tolerance for MLP activations


def _load_stack(convs, bns, ws, dev):
    with torch.no_grad():
        for conv, bn, (w, b, g, bt) in zip(convs, bns, ws):
            conv.weight.copy_(torch.from_numpy(w).reshape(conv.weight.shape))
            conv.bias.copy_(torch.from_numpy(b))
            bn.weight.copy_(torch.from_numpy(g))
            bn.bias.copy_(torch.from_numpy(bt))


@pytest.mark.parametrize("B,N,npoint,radius,nsample,D,mlp", [
    (2, 1024, 128, 0.2, 32, 0, [64, 64, 128]),        # SA1-shaped (no features)
    (2, 512, 64, 0.4, 64, 128, [128, 128, 256]),       # SA2-shaped (131 input channels)
    (3, 300, 20, 0.3, 16, 5, [32, 48, 20]),            # ragged everything: odd N, D%4!=0, Cout%32!=0
    (1, 256, 16, 0.25, 8, 3, [16]),                    # single layer stack
])
def test_sa_forward_vs_oracle(dev, B, N, npoint, radius, nsample, D, mlp):
    x = make_clouds(B, N, 77 + N)
    st = make_start_idx(B, N, 3)
    rng = np.random.default_rng(9)
    pts = rng.normal(size=(B, D, N)).astype(np.float32) if D else None
    ws = seeded_weights([D + 3] + mlp, 5)
    ora = R.PointNetSetAbstraction(npoint, radius, nsample, D + 3, mlp, False, ws)
    ref_xyz, ref32, acts = ora.forward(x, pts, st, f64=False, return_all=True)
    _, ref64 = ora.forward(x, pts, st, f64=True)
    layer = PointNetSetAbstraction(npoint, radius, nsample, D + 3, mlp, False).to(dev)
    _load_stack(layer.mlp_convs, layer.mlp_bns, ws, dev)
    got_xyz, got = layer(torch.from_numpy(x).to(dev), None if pts is None else torch.from_numpy(pts).to(dev),
                         torch.from_numpy(st).to(dev))
    assert tuple(got_xyz.shape) == (B, 3, npoint) and tuple(got.shape) == (B, mlp[-1], npoint)
    assert np.array_equal(got_xyz.cpu().numpy(), ref_xyz)
    e64 = assert_close(got.detach().cpu().numpy(), ref64, REL, "vs f64 oracle")
    e32 = assert_close(got.detach().cpu().numpy(), ref32, REL, "vs f32 oracle")
    print("rel err vs f64 %.2e, vs f32 %.2e" % (e64, e32))


def test_sa_group_all_vs_oracle(dev):
    B, N, D = 2, 128, 256
    x = make_clouds(B, N, 5)
    rng = np.random.default_rng(1)
    pts = rng.normal(size=(B, D, N)).astype(np.float32)
    mlp = [256, 512, 1024]
    ws = seeded_weights([D + 3] + mlp, 6)
    ora = R.PointNetSetAbstraction(None, None, None, D + 3, mlp, True, ws)
    ref_xyz, ref64 = ora.forward(x, pts, f64=True)
    layer = PointNetSetAbstraction(None, None, None, D + 3, mlp, True).to(dev)
    _load_stack(layer.mlp_convs, layer.mlp_bns, ws, dev)
    got_xyz, got = layer(torch.from_numpy(x).to(dev), torch.from_numpy(pts).to(dev))
    assert np.array_equal(got_xyz.cpu().numpy(), ref_xyz)
    assert_close(got.detach().cpu().numpy(), ref64, REL, "group_all vs f64 oracle")


def test_sa_msg_vs_oracle(dev):
    B, N, S = 2, 1024, 128
    x = make_clouds(B, N, 15)
    st = make_start_idx(B, N, 4)
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(B, 3, N)).astype(np.float32)
    radii, ks, mlps = [0.1, 0.2, 0.4], [16, 32, 64], [[32, 32, 64], [64, 64, 128], [64, 96, 128]]
    ws = [seeded_weights([6] + m, 20 + i) for i, m in enumerate(mlps)]
    ora = R.PointNetSetAbstractionMsg(S, radii, ks, 3, mlps, ws)
    ref_xyz, ref64 = ora.forward(x, pts, st, f64=True)
    layer = PointNetSetAbstractionMsg(S, radii, ks, 3, mlps).to(dev)
    for i in range(3):
        _load_stack(layer.conv_blocks[i], layer.bn_blocks[i], ws[i], dev)
    got_xyz, got = layer(torch.from_numpy(x).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(st).to(dev))
    assert tuple(got.shape) == (B, 320, S)
    assert np.array_equal(got_xyz.cpu().numpy(), ref_xyz)
    assert_close(got.detach().cpu().numpy(), ref64, REL, "MSG vs f64 oracle")


@pytest.mark.parametrize("B,N,S,K,D,mlp,xyz_first,use_idx", [
    (2, 512, 64, 32, 0, [64, 64, 128], True, True),
    (2, 256, 32, 16, 128, [128, 64], True, True),
    (2, 256, 32, 16, 12, [32, 40, 24], False, True),     # MSG channel order, ragged widths
    (2, 128, 1, 128, 64, [64, 128], True, False),          # group_all: identity rows
    (1, 200, 10, 8, 6, [16], True, True),                  # single-layer stack (MAX-mode dY with GROUP input)
    (4, 1024, 256, 32, 0, [64, 64, 128], True, True),      # M = 32768 rows: large enough for the opt-in sparse-max dX (PAPC_SPARSE_MAX=1)
    (2, 512, 64, 32, 4, [32, 32, 64], False, True),        # 7 input channels (normals padded to four + xyz, MSG order): streaming first-layer dW
    (2, 512, 64, 16, 4, [64, 96, 128], True, True),        # ... SSG column order
])
@pytest.mark.parametrize("seed", [40, 41, 42, 43])
def test_stack_backward_vs_torch(dev, B, N, S, K, D, mlp, xyz_first, use_idx, seed):
    x = make_clouds(B, N, 31 + N)
    xyz = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    st = torch.from_numpy(make_start_idx(B, N, 1)).to(dev)
    rng = np.random.default_rng(8)
    feats = torch.from_numpy(rng.normal(size=(B, N, D)).astype(np.float32)).to(dev) if D else None
    if use_idx:
        _, new_xyz = F._fps_raw(xyz, S, st)
        idx = F._ball_query_raw([0.3], [K], xyz, new_xyz)[0]
    else:
        new_xyz = torch.zeros(B, 1, 3, device=dev)
        idx = None
    # (arbitrary weight seeds: the float64 reference below takes the kernel's own max / ReLU decisions, so near-ties -- where an fp32
    # kernel and a float64 chain legitimately pick differently -- neither hide nor fake an arithmetic error; torch_ref.stack_routed)
    ws = seeded_weights([D + 3] + mlp, seed)
    params = []
    for (w, b, g, bt) in ws:
        params += [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (w, b, g, bt)]
    if feats is not None:
        feats.requires_grad_(True)
    spec = StackSpec(B, N, S, K, D, xyz_first)
    out = shared_mlp_max(spec, None, xyz, new_xyz, feats, idx, params)
    from tests.util import kernel_decisions
    argmax, alive, masks = kernel_decisions(out)
    gout = torch.from_numpy(rng.normal(size=tuple(out.shape)).astype(np.float32)).to(dev)
    out.backward(gout)

    # float64 torch reference on the same indices, routed through the kernel's own decisions
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    f64 = feats.detach().double().requires_grad_(True) if feats is not None else None
    ridx = idx if idx is not None else torch.arange(N, device=dev).view(1, 1, N).expand(B, 1, N)
    rows = torch_ref.group(xyz.double(), new_xyz.double(), f64, ridx, xyz_first).reshape(B * S * K, D + 3)
    ref, stats = torch_ref.stack_routed(rows, [tuple(p64[4 * l:4 * l + 4]) for l in range(len(mlp))], K, 1e-5, argmax, alive, masks)
    print("decisions that differ from float64's own:", stats)
    assert_close(out.detach().cpu().numpy(), ref.detach().cpu().numpy(), REL, "stack forward")
    ref.backward(gout.double())
    names = ["w", "b", "gamma", "beta"]
    # weight gradients are sums over all M rows with heavy cancellation (max|dW| << sum|terms|): the fp32 accumulation error relative
    # to max|dW| grows like sqrt(M); measured 1e-6 .. 3e-6 on every flavour at 32768 rows (plain torch fp32 autograd: up to 9e-6)
    gtol = 2e-4
    for l in range(len(mlp)):
        for j in range(4):
            got, want = params[4 * l + j].grad, p64[4 * l + j].grad
            if j == 1:
                # conv bias feeds a train-mode BN: its true gradient is exactly zero; both sides hold rounding noise
                scale = float(p64[4 * l].grad.abs().max())
                assert float(got.abs().max()) <= 1e-4 * scale, "db layer %d not ~0" % l
                continue
            assert_close(got.cpu().numpy(), want.cpu().numpy(), gtol, "d%s layer %d" % (names[j], l))
    if feats is not None:
        assert_close(feats.grad.cpu().numpy(), f64.grad.cpu().numpy(), 2e-4, "dfeats")


@pytest.mark.parametrize("D,K", [(0, 32), (16, 64)])
def test_max_layer_without_stored_output_vs_stored_and_f64(dev, D, K):
    """The max-pooled last layer (64 -> 128) whose [M, 128] output is never written (papc_mlp_max_nostore_ok: forward keeps the per-group
    extrema only, dX = [P | A] wcat^T, dW from T = P'^T A, the input rows' Gram matrix and their column sums): the pooled output is
    bit-identical to the stored-output path (same kernel minus the store), every gradient within 2e-4 of float64 torch and of the
    stored-output path, with and without in-place gradient targets."""
    from papc_amd import mlp as M_
    B, N, S, mlp = 8, 1024, 8192 // K, [64, 64, 128]
    x = make_clouds(B, N, 77)
    xyz = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    st = torch.from_numpy(make_start_idx(B, N, 1)).to(dev)
    rng = np.random.default_rng(9)
    feats0 = torch.from_numpy(rng.normal(size=(B, N, D)).astype(np.float32)).to(dev) if D else None
    _, new_xyz = F._fps_raw(xyz, S, st)
    idx = F._ball_query_raw([0.3], [K], xyz, new_xyz)[0]
    ws = seeded_weights([D + 3] + mlp, 41)
    assert _lib.load().papc_mlp_max_nostore_ok(B * S * K, 64, 128, K) == 1

    def run(nostore, targets):
        params = []
        for (w, b, g, bt) in ws:
            params += [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (w, b, g, bt)]
        feats = feats0.clone().requires_grad_(True) if D else None
        spec = StackSpec(B, N, S, K, D, True)
        tg = None
        if targets:
            tg = [torch.ones_like(p) for p in params]
            spec.grad_targets = tg
        old = M_._NOSTORE
        M_._NOSTORE = nostore
        try:
            if targets:     # (shared_mlp_max derives the targets from the parameters' own flags: set them on the spec, call the Function)
                out = SharedMLPStack.apply(spec, None, xyz, new_xyz, feats, idx, None, *params)
            else:
                out = shared_mlp_max(spec, None, xyz, new_xyz, feats, idx, params)
        finally:
            M_._NOSTORE = old
        assert bool(out.grad_fn.nostore) == nostore
        gout = torch.from_numpy(np.random.default_rng(10).normal(size=tuple(out.shape)).astype(np.float32)).to(dev)
        out.backward(gout)
        if targets:
            grads = [None if j % 4 == 1 else (t - 1.0) for j, t in enumerate(tg)]
            assert all(params[j].grad is None for j in range(len(params)) if j % 4 != 1)
        else:
            grads = [p.grad for p in params]
        return out.detach(), grads, (feats.grad if D else None), params, gout

    out_n, g_n, gf_n, params, gout = run(True, False)
    out_s, g_s, gf_s, _, _ = run(False, False)
    _, g_t, _, _, _ = run(True, True)
    assert torch.equal(out_n, out_s)
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    f64 = feats0.double().requires_grad_(True) if D else None
    rows = torch_ref.group(xyz.double(), new_xyz.double(), f64, idx, True).reshape(B * S * K, D + 3)
    ref = torch_ref.stack_max(rows, [tuple(p64[4 * l:4 * l + 4]) for l in range(3)], K, 1e-5)
    assert_close(out_n.cpu().numpy(), ref.detach().cpu().numpy(), REL, "forward")
    ref.backward(gout.double())
    names = ["w", "b", "gamma", "beta"]
    for l in range(3):
        for j in (0, 2, 3):
            want = p64[4 * l + j].grad.cpu().numpy()
            assert_close(g_n[4 * l + j].cpu().numpy(), want, 2e-4, "no-store d%s layer %d vs f64" % (names[j], l))
            assert_close(g_n[4 * l + j].cpu().numpy(), g_s[4 * l + j].cpu().numpy(), 2e-4, "no-store vs stored d%s layer %d" % (names[j], l))
            assert_close(g_t[4 * l + j].reshape(want.shape).cpu().numpy(), want, 2e-4, "no-store in-place d%s layer %d" % (names[j], l))
        assert g_n[4 * l + 1] is None or float(g_n[4 * l + 1].abs().max()) == 0.0 or l < 2
    if D:
        assert_close(gf_n.cpu().numpy(), f64.grad.cpu().numpy(), 2e-4, "dfeats")
        assert_close(gf_n.cpu().numpy(), gf_s.cpu().numpy(), 2e-4, "dfeats vs stored")


def test_full_size_sa1_properties(dev):
    """BASELINE config 2, SA1 at full size (B=32, N=4096): BN'd output is a max over K -> invariant to permuting
    the nsample slots, and equal for duplicated (padded) neighbour lists; checked through shuffled idx."""
    B, N, S, K = 32, 4096, 512, 32
    x = torch.from_numpy(make_clouds(B, N, 1234)).to(dev)
    xyz = x.transpose(1, 2)
    st = torch.from_numpy(make_start_idx(B, N, 1234)).to(dev)
    _, new_xyz = F._fps_raw(xyz, S, st)
    idx = F._ball_query_raw([0.2], [K], xyz, new_xyz)[0]
    ws = seeded_weights([3, 64, 64, 128], 1)
    params = [torch.from_numpy(a).to(dev) for tup in ws for a in tup]
    spec = StackSpec(B, N, S, K, 0, True)
    out1 = shared_mlp_max(spec, None, xyz, new_xyz, None, idx, params)
    perm = torch.randperm(K, device=dev)
    out2 = shared_mlp_max(spec, None, xyz, new_xyz, None, idx[:, :, perm].contiguous(), params)
    assert torch.isfinite(out1).all()
    assert_close(out2.cpu().numpy(), out1.cpu().numpy(), 1e-5, "slot-permutation invariance")
    out3 = shared_mlp_max(spec, None, xyz, new_xyz, None, idx, params)
    assert torch.equal(out1, out3)                     # deterministic: no atomics in the forward


def test_inplace_grad_accumulation_matches_autograd_path(dev):
    """With pre-allocated contiguous .grad tensors (FlatParams) the backward adds gradients in place and returns None
    to autograd; the result must equal the ordinary autograd-accumulated gradients (and really accumulate)."""
    B, N = 2, 512
    x = torch.from_numpy(make_clouds(B, N, 9)).to(dev)
    st = torch.from_numpy(make_start_idx(B, N, 9)).to(dev)
    torch.manual_seed(1)
    a = PointNetSetAbstraction(64, 0.3, 16, 3, [32, 64], False).to(dev)
    b = PointNetSetAbstraction(64, 0.3, 16, 3, [32, 64], False).to(dev)
    b.load_state_dict(a.state_dict())
    fired = []
    for name, p in b.named_parameters():
        p.grad = torch.ones_like(p)                      # pre-existing gradient: the in-place path must ADD to it ...
        p._papc_inplace_grad = True                      # ... which a parameter takes only when it opted in (nodeparts.grad_targets_of)
        p.register_hook(lambda g_, n=name: fired.append(n) if g_ is not None else None)    # (the engine calls a leaf's hook with None for an undefined gradient)
    _, oa = a(x, None, st)
    _, ob = b(x, None, st)
    assert torch.equal(oa, ob)
    g = torch.randn_like(oa)
    oa.backward(g)
    ob.backward(g)
    torch.cuda.synchronize()
    # the nodes hand autograd None for a gradient they added in place: a hook that sees a tensor means the autograd path was taken after all
    assert not fired, "gradients went back through autograd: %s" % fired
    for (name, pa), pb in zip(a.named_parameters(), b.parameters()):
        # the same kernels on the same operands, then ONE fp32 add per element (every fold job ends in *o + s): the bits of 1 + g.  That holds for
        # the conv biases under the train-mode BN too (true gradient 0: both sides fold the same rounding noise)
        assert torch.equal(pb.grad, 1.0 + pa.grad), name


def test_full_size_config3_msg_sa1(dev):
    """BASELINE config 3 (PointNet++ MSG segment SA1: B=16, N=2048, radii 0.1/0.2/0.4, K=32/64/128, in_channel 3+3):
    neighbour lists index-exact vs the C oracle at full size; MLP output checked through size-independent
    properties (finite, deterministic, branch concat order) and, branch by branch at full size, against the f64 oracle."""
    B, N, S = 16, 2048, 512
    x = make_clouds(B, N, 33)
    st = make_start_idx(B, N, 33)
    radii, ks, mlps = [0.1, 0.2, 0.4], [32, 64, 128], [[32, 32, 64], [64, 64, 128], [64, 96, 128]]
    ws = [seeded_weights([6] + m, 50 + i) for i, m in enumerate(mlps)]
    layer = PointNetSetAbstractionMsg(S, radii, ks, 3, mlps).to(dev)
    for i in range(3):
        _load_stack(layer.conv_blocks[i], layer.bn_blocks[i], ws[i], dev)
    tx = torch.from_numpy(x).to(dev)
    xyz = np.ascontiguousarray(x.transpose(0, 2, 1))
    fps = R.farthest_point_sample(xyz, S, st)
    new_xyz = R.index_points(xyz, fps)
    got_idx = F._ball_query_raw(radii, ks, tx.transpose(1, 2), torch.from_numpy(new_xyz).to(dev))
    for r, k, gi in zip(radii, ks, got_idx):
        assert np.array_equal(gi.cpu().numpy().astype(np.int64), R.query_ball_point(r, k, xyz, new_xyz))
    out_xyz, out = layer(tx, tx, torch.from_numpy(st).to(dev))     # points = xyz (3 extra channels), as the seg model feeds it
    assert tuple(out.shape) == (B, 320, S) and torch.isfinite(out).all()
    assert np.array_equal(out_xyz.cpu().numpy(), new_xyz.transpose(0, 2, 1))
    _, out2 = layer(tx, tx, torch.from_numpy(st).to(dev))
    assert torch.equal(out, out2)
    # batch statistics couple the clouds, so the oracle comparison needs the full batch: ALL THREE branches at full size (K = 32 / 64 / 128:
    # 0.26 / 0.52 / 1.05 M rows -- the 64- and 128-neighbour branches are 80 % of SA1's FLOPs), each held to the float64 oracle on its own
    # slice of the concatenated output (pointnet2_basic_layers.py:280: branch order = radius order)
    ora = R.PointNetSetAbstractionMsg(S, radii, ks, 3, mlps, ws)
    _, ref = ora.forward(x, x, st, f64=True)
    got = out.detach().cpu().numpy()
    c0 = 0
    for r, k, m in zip(radii, ks, mlps):
        assert_close(got[:, c0:c0 + m[-1]], ref[:, c0:c0 + m[-1]], REL, "config-3 SA1 branch r=%.1f K=%d %s vs f64 oracle (full size)" % (r, k, m))
        c0 += m[-1]
    assert c0 == 320


def test_full_size_config3_msg_sa2_196_branch(dev):
    """BASELINE config 3, the second SA2 branch at full size (B=16, 512 -> 128 centroids, r = 0.8, K = 128, 320 + 3 -> 128 -> 196 -> 256,
    M = 262 144 rows; segment/pointnet2/pointnet2.py:63): the ragged flavours of the row-streaming kernels (196 = 12 k blocks + 4
    channels / 6 column tiles + 4 columns) against the float64 oracle at the size the bench runs, and their gradients against the tiled
    kernels' (PAPC_STREAM=0, PAPC_DW_ROWSX=0: other kernels, same exact-split products)."""
    B, N, S, K, D = 16, 512, 128, 128, 320
    mlp = [128, 196, 256]
    rng = np.random.default_rng(77)
    x = make_clouds(B, N, 77)[:, :3]
    feats = rng.normal(size=(B, D, N)).astype(np.float32)
    st = make_start_idx(B, N, 77)
    ws = [seeded_weights([D + 3] + mlp, 91)]
    gout = torch.from_numpy(rng.normal(size=(B, mlp[-1], S)).astype(np.float32)).to(dev)

    def run(knobs):
        lib = _lib.load()
        old = {}
        for n, v in knobs.items():
            o = _lib.ctypes.c_int(0)
            _lib.check(lib.papc_knob_get(n.encode(), _lib.ctypes.byref(o)), "papc_knob_get")
            old[n] = o.value
            _lib.check(lib.papc_knob_set(n.encode(), v), "papc_knob_set")
        try:
            layer = PointNetSetAbstractionMsg(S, [0.8], [K], D, [mlp]).to(dev)
            _load_stack(layer.conv_blocks[0], layer.bn_blocks[0], ws[0], dev)
            tf = torch.from_numpy(feats).to(dev).requires_grad_(True)
            _, out = layer(torch.from_numpy(x).to(dev), tf, torch.from_numpy(st).to(dev))
            out.backward(gout)
            torch.cuda.synchronize()
            grads = [p.grad.detach().cpu().numpy() for n_, p in layer.named_parameters() if not n_.endswith("bias") or "bn_blocks" in n_]
            return out.detach().cpu().numpy(), grads, tf.grad.cpu().numpy()
        finally:
            for n, v in old.items():
                _lib.check(lib.papc_knob_set(n.encode(), v), "papc_knob_set")

    out, grads, gf = run({})
    assert out.shape == (B, mlp[-1], S) and np.isfinite(out).all()
    ora = R.PointNetSetAbstractionMsg(S, [0.8], [K], D, [mlp], ws)
    _, ref = ora.forward(x, feats, st, f64=True)
    assert_close(out, ref, REL, "config-3 SA2 branch [128, 196, 256] vs f64 oracle (full size)")
    out_t, grads_t, gf_t = run({"PAPC_STREAM": 0, "PAPC_DW_ROWSX": 0})
    assert_close(out, out_t, 2e-6, "ragged stream kernels vs tiled, forward")
    for a_, b_ in zip(grads, grads_t):
        assert_close(a_, b_, 1e-4, "ragged stream / row-streaming dW vs tiled, parameter gradients")
    assert_close(gf, gf_t, 1e-4, "ragged stream vs tiled, feature gradient")


@pytest.mark.parametrize("env", [
    {"PAPC_GEMM_F32": "1", "PAPC_DW_F32": "1"},   # the exact-fp32 MFMA flavour (v_mfma_f32_32x32x2_f32) of every GEMM
    {"PAPC_GEMM_WS": "3"},                        # the opt-in wave-specialised forward / dX GEMM
    {"PAPC_GEMM_TL": "1"},                        # the opt-in transposed-accumulator dX epilogue
    {"PAPC_SPARSE_MAX": "1"},                     # the opt-in dX of the max-pooled layer that never reads its dense output
])
def test_alternative_kernel_flavours(dev, env):
    """The kernel flavours are chosen once per process from the environment, so the alternatives are held to the same
    parity tests in a child process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_mlp.py", "-q", "-m", "gpu", "-x",
                        "-k", "sa_forward or group_all or msg_vs or stack_backward"], cwd=root, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]


def test_backward_near_ties_explain_the_seed40_excess(dev):
    """The M = 32768 backward case uses weight seed 41 because seed 40 gives ~1e-3 .. 1e-2 on dW; the claimed cause is a
    pooled (group, channel) decision within fp32 rounding of a tie, where the fp32 kernels and the float64 reference may
    legitimately decide differently: WHICH row wins the max, and whether the winner is barely alive (z > 0) or dead.  Tested
    here instead of asserted:
    (i) the kernel's pooled output is within 1e-5 of the float64 max everywhere, and wherever its winner cannot be the float64
        winner the two candidates differ by <= 1e-5 of the activation scale;
    (ii) with the float64 reference routed through the kernel's decisions (winner row; alive iff the kernel's output is > 0),
        every gradient agrees to the usual 2e-4 -- or, where the sum is ill conditioned (the first layer's weight gradient:
        3 input channels, 32768 cancelling rows, ReLU decisions of the two layers above within rounding of 0), to three times
        what PLAIN fp32 torch autograd loses on the same routed graph: the excess is a property of fp32, not of the kernels."""
    B, N, S, K, mlp = 4, 1024, 256, 32, [64, 64, 128]
    x = make_clouds(B, N, 31 + N)
    xyz = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    st = torch.from_numpy(make_start_idx(B, N, 1)).to(dev)
    _, new_xyz = F._fps_raw(xyz, S, st)
    idx = F._ball_query_raw([0.3], [K], xyz, new_xyz)[0]
    ws = seeded_weights([3] + mlp, 40)
    params = []
    for (w, b, g, bt) in ws:
        params += [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (w, b, g, bt)]
    spec = StackSpec(B, N, S, K, 0, True)
    out = shared_mlp_max(spec, None, xyz, new_xyz, None, idx, params)
    rng = np.random.default_rng(8)
    gout = torch.from_numpy(rng.normal(size=tuple(out.shape)).astype(np.float32)).to(dev)
    from tests.util import kernel_decisions
    kernel_argmax = kernel_decisions(out)[0].clone()                            # [B*S, C] int32: kept by the stack node for its backward
    assert kernel_argmax.dtype == torch.int32 and tuple(kernel_argmax.shape) == (B * S, mlp[-1])
    out.backward(gout)
    o = out.detach().double()

    def reference(dt):
        """the stack in torch at precision dt, pooled through the KERNEL's decisions (winner row; alive iff its output > 0)"""
        ps = [p.detach().to(dt).requires_grad_(True) for p in params]
        act = torch_ref.group(xyz.to(dt), new_xyz.to(dt), None, idx, True).reshape(B * S * K, 3)
        z = None
        for l in range(3):
            w, b, g, bt = ps[4 * l: 4 * l + 4]
            y = act @ w.t() + b
            z = (y - y.mean(0)) / torch.sqrt(y.var(0, unbiased=False) + 1e-5) * g + bt
            act = torch.relu(z)
        z = z.reshape(B * S, K, mlp[-1])                                        # pre-ReLU values of the pooled layer
        true_max = torch.relu(z).max(1).values.detach().double()
        tol = 1e-5 * float(true_max.abs().max())
        route = kernel_argmax.long().unsqueeze(1)                               # the row the kernel sent the gradient to
        zr = z.gather(1, route).squeeze(1)
        assert bool((torch.relu(zr.detach()).double() >= true_max - tol).all()), "a kernel winner is not within 1e-5 of the max"
        alive = o > 0
        routed = torch.where(alive, zr, torch.zeros_like(zr))
        routed.backward(gout.to(dt))
        return ps, z.detach(), zr.detach().double(), route, alive, true_max, tol

    p64, z, zr, route, alive, true_max, tol = reference(torch.float64)
    assert_close(out.detach().cpu().numpy(), true_max.cpu().numpy(), REL, "forward, seed 40")
    assert bool((zr[alive] > -tol).all()) and bool((zr[~alive] < tol).all()), "a pooling decision outside the tie margin"
    flips = int((alive != (zr > 0)).sum())
    moved = int((route.squeeze(1) != torch.relu(z).argmax(1)).sum())
    p32 = reference(torch.float32)[0]
    bad = []
    print("seed 40: %d alive/dead decisions and %d winner rows differ from float64 (of %d)" % (flips, moved, alive.numel()))
    for l in range(3):
        for j, nm in enumerate(["w", "b", "gamma", "beta"]):
            if j == 1:
                continue
            want = p64[4 * l + j].grad
            e32 = float((p32[4 * l + j].grad.double() - want).abs().max() / want.abs().max())
            ours = float((params[4 * l + j].grad.double() - want).abs().max() / want.abs().max())
            print("   d%s layer %d: kernels %.2e, plain fp32 torch autograd %.2e (of max|grad|)" % (nm, l, ours, e32))
            bad.append((ours <= max(2e-4, 3.0 * e32), "seed 40 d%s layer %d: %.2e vs plain fp32 autograd %.2e" % (nm, l, ours, e32)))
    assert all(ok for ok, _ in bad), [m for ok, m in bad if not ok]


@pytest.mark.parametrize("mlp", [[64, 64, 128], [64, 128, 128]])
def test_xyz_first_layer_gram_path_vs_rows_and_f64(dev, mlp):
    """SA1 of the classifiers (coordinates only, pointnet2_basic_layers.py:152-153): the first layer run through its input moments
    (csrc/xyz1.hip -- no [M, 64] output, BN statistics and the layer's whole backward in closed form, the layer folded into the
    second one's operand) against (a) the row kernels that materialise it and (b) float64 torch: forward 1e-5, every gradient
    2e-4, running statistics equal, in-place gradient targets honoured."""
    from papc_amd import mlp as M_
    B, N, S, K = 8, 1024, 256, 32                       # M = 65536 rows: the smallest problem the streaming kernels take
    x = make_clouds(B, N, 77)
    xyz = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    st = torch.from_numpy(make_start_idx(B, N, 5)).to(dev)
    _, new_xyz = F._fps_raw(xyz, S, st)
    idx = F._ball_query_raw([0.25], [K], xyz, new_xyz)[0]
    ws = seeded_weights([3] + mlp, 43)
    rng = np.random.default_rng(3)
    res = {}
    for flag in (True, False):
        params = [torch.from_numpy(a).to(dev).requires_grad_(True) for tup in ws for a in tup]
        bufs = [(torch.zeros(c, device=dev), torch.ones(c, device=dev)) for c in mlp]
        old = M_._XYZ1
        M_._XYZ1 = flag
        try:
            out = shared_mlp_max(StackSpec(B, N, S, K, 0, True), bufs, xyz, new_xyz, None, idx, params)
        finally:
            M_._XYZ1 = old
        assert out.grad_fn.xyz1 == flag, "the Gram path must be taken exactly when enabled"
        gout = torch.from_numpy(np.random.default_rng(9).normal(size=tuple(out.shape)).astype(np.float32)).to(dev)
        out.backward(gout)
        res[flag] = (out.detach(), [p.grad for p in params], bufs, params, gout)
    out, grads, bufs, params, gout = res[True]
    out_r, grads_r, bufs_r, _, _ = res[False]
    assert_close(out.cpu().numpy(), out_r.cpu().numpy(), 2e-6, "gram path vs rows forward")
    for (rm, rv), (rm_r, rv_r) in zip(bufs, bufs_r):
        assert_close(rm.cpu().numpy(), rm_r.cpu().numpy(), 1e-5, "running mean")
        assert_close(rv.cpu().numpy(), rv_r.cpu().numpy(), 1e-5, "running var")
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    rows = torch_ref.group(xyz.double(), new_xyz.double(), None, idx, True).reshape(B * S * K, 3)
    ref = torch_ref.stack_max(rows, [tuple(p64[4 * l:4 * l + 4]) for l in range(3)], K, 1e-5)
    assert_close(out.cpu().numpy(), ref.detach().cpu().numpy(), REL, "gram path forward vs f64")
    ref.backward(gout.double())
    for l in range(3):
        for j, nm in enumerate(["w", "b", "gamma", "beta"]):
            if j == 1:
                assert grads[4 * l + j] is None or float(grads[4 * l + j].abs().max()) <= 1e-4 * float(p64[4 * l].grad.abs().max())
                continue
            assert_close(grads[4 * l + j].cpu().numpy(), p64[4 * l + j].grad.cpu().numpy(), 2e-4, "gram path d%s layer %d vs f64" % (nm, l))
            # (sanity only: the row kernels take their ReLU / max decisions from MFMA-computed activations, the Gram path from fma chains --
            # decisions within rounding of a tie differ, which moves a max-pooled gradient by up to ~1e-2, tests/test_gpu_step.py)
            assert_close(grads[4 * l + j].cpu().numpy(), grads_r[4 * l + j].cpu().numpy(), 3e-2, "gram path d%s layer %d vs rows" % (nm, l))
    # in-place targets: added on top of what the buffers hold
    tg = [torch.ones_like(p) for p in params]
    spec = StackSpec(B, N, S, K, 0, True)
    spec.grad_targets = tg
    o3 = SharedMLPStack.apply(spec, None, xyz, new_xyz, None, idx, None, *params)
    for p in params:
        p.grad = None
    o3.backward(gout)
    for l in range(3):
        for j in (0, 2, 3):
            assert params[4 * l + j].grad is None
            assert torch.allclose(tg[4 * l + j] - 1.0, grads[4 * l + j].reshape(tg[4 * l + j].shape), rtol=1e-4, atol=3e-6), (l, j)


@pytest.mark.parametrize("D,K,mlp", [(0, 32, [64, 64, 128]), (128, 64, [128, 128, 256])])
def test_twelve_wave_dx_flavours_match_eight(dev, D, K, mlp):
    """Two row-streaming dX flavours run twelve waves per workgroup (three per SIMD; stream_kernel<..., 12>, PAPC_STREAM_NW12): the dX folded into a
    coordinates-only first layer's sums and the padded max layer's 256 -> 128.  Same products; the tiles reach a lane's running sums in another
    order, so the gradients agree to rounding with the eight-wave launch (pointnet2_basic_layers.py:215-219 backward)."""
    B, N, S = 8, 1024, 8192 // K * (2 if K == 64 else 1)
    x = make_clouds(B, N, 78)
    xyz = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    st = torch.from_numpy(make_start_idx(B, N, 2)).to(dev)
    rng = np.random.default_rng(19)
    feats0 = torch.from_numpy(rng.normal(size=(B, N, D)).astype(np.float32)).to(dev) if D else None
    _, new_xyz = F._fps_raw(xyz, S, st)
    idx = F._ball_query_raw([0.3], [K], xyz, new_xyz)[0]
    ws = seeded_weights([D + 3] + mlp, 43)
    gout = None
    res = {}
    lib = _lib.load()
    for nw12 in (1, 0):
        _lib.check(lib.papc_knob_set(b"PAPC_STREAM_NW12", nw12), "papc_knob_set")
        try:
            params = []
            for (w, b, g, bt) in ws:
                params += [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (w, b, g, bt)]
            feats = feats0.clone().requires_grad_(True) if D else None
            spec = StackSpec(B, N, S, K, D, True)
            out = shared_mlp_max(spec, None, xyz, new_xyz, feats, idx, params)
            if gout is None:
                gout = torch.from_numpy(np.random.default_rng(20).normal(size=tuple(out.shape)).astype(np.float32)).to(dev)
            out.backward(gout)
            torch.cuda.synchronize()
            res[nw12] = (out.detach().cpu().numpy(), [p.grad.cpu().numpy() for j, p in enumerate(params) if j % 4 != 1],
                         feats.grad.cpu().numpy() if D else None)
        finally:
            _lib.check(lib.papc_knob_set(b"PAPC_STREAM_NW12", 1), "papc_knob_set")
    assert np.array_equal(res[1][0], res[0][0])
    for a_, b_ in zip(res[1][1], res[0][1]):
        assert_close(a_, b_, 2e-5, "twelve-wave vs eight-wave dX: parameter gradients")
    if D:
        assert_close(res[1][2], res[0][2], 2e-5, "twelve-wave vs eight-wave dX: feature gradient")


def test_group_max_sign_hint_is_bit_identical(dev, monkeypatch):
    """papc_group_max.sign_src (the layer's gamma): the fused group max follows one extremum per channel -- the max where gamma >= 0, the min
    elsewhere (seeded_weights draws a quarter of the gammas negative) -- and writes it to both pairs of arrays.  papc_bn_select_max_f32 picks the
    same value either way: output and gradients have the bits of the two-extrema epilogue (PAPC_GSIGN=0 / PAPC_SA_NO_GSIGN;
    pointnet2_basic_layers.py:215-219)."""
    B, N, K, mlp = 8, 1024, 32, [64, 64, 128]
    S = 8192 // K
    x = make_clouds(B, N, 79)
    xyz = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    st = torch.from_numpy(make_start_idx(B, N, 3)).to(dev)
    _, new_xyz = F._fps_raw(xyz, S, st)
    idx = F._ball_query_raw([0.3], [K], xyz, new_xyz)[0]
    ws = seeded_weights([3] + mlp, 47)
    assert any((g < 0).any() for (_, _, g, _) in ws)
    gout = None
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PAPC_GSIGN", mode)
        params = []
        for (w, b, g, bt) in ws:
            params += [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (w, b, g, bt)]
        out = shared_mlp_max(StackSpec(B, N, S, K, 0, True), None, xyz, new_xyz, None, idx, params)
        if gout is None:
            gout = torch.from_numpy(np.random.default_rng(21).normal(size=tuple(out.shape)).astype(np.float32)).to(dev)
        out.backward(gout)
        torch.cuda.synchronize()
        res[mode] = (out.detach().cpu().numpy(), [p.grad.cpu().numpy() for j, p in enumerate(params) if j % 4 != 1])
    assert np.array_equal(res["1"][0], res["0"][0])
    for a_, b_ in zip(res["1"][1], res["0"][1]):
        assert np.array_equal(a_, b_)
