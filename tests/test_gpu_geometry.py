"""The launch geometries the chip-sized thresholds pick -- at test-sized shapes, through the run-time knobs (papc_knob_set).

The GEMM, gather-add and FPS launchers choose a kernel flavour and a grid from thresholds sized for 256 CUs: at a thousand rows they
always take the "small problem" flavour, one tile per workgroup.  Here the thresholds are scaled DOWN instead of the shapes up, so the
flavours the benchmark runs (128 x 128 tile, 16-deep k stages, a persistent loop over several row tiles with a ragged last one, the
row-streaming kernels on a capped grid, gather-add workgroups whose boundaries cut groups, all 25 FPS geometries) are each held to the
float64 reference AND to the default geometry on the same input.

    against float64 (tests/torch_ref.py::stack_routed on the kernel's own max / ReLU decisions): forward 1e-5, gradients 2e-4
    against the default knobs: forward 2e-6, gradients 2e-5 ("same products, another order of the BatchNorm partial sums")

Why each test can fail (read from the kernels):
  * PAPC_PARTS=3 on P4 (7 row tiles, the last of 120 rows): a workgroup walks tiles b, b + 3, b + 6; if the tile advance of gemm_kernel's
    fetch cursor (tile_f += gridDim.x, the row contexts and neighbour prefetch that go with it) or of its compute cursor were wrong, rows
    of a later tile would be computed from another tile's operands or never stored -- the forward misses 1e-5 by orders of magnitude.
  * PAPC_LG_PARTS=3 (342 rows per workgroup, groups of 16): lingather_bwd_kernel keeps the pending sum of a group's padding duplicates in
    registers; a group cut by a workgroup boundary must be flushed by BOTH workgroups.  Dropping the pending state at the boundary loses
    those rows' share of dfeats / dW (the groups at the boundaries consist of one repeated index: all but one of their rows are pending).
  * an FPS geometry whose tie order is not first-maximum picks another index on the lattice, where the maximum is shared among lanes, DPP
    rows and waves in most iterations.
Knobs are process-global: one fixture restores every knob this file touches.

Measured on the MI355X, worst over the file: 4.16e-7 / 1.25e-6 against the default geometry (forward / gradients), 6.27e-7 / 1.22e-6
against float64.  (Setting A on G1 -- 4096 rows on ONE workgroup -- measured 2.58e-6 against the 2e-6 forward bar while gemm_kernel carried
one fp32 statistics chain over all the row tiles of a workgroup; it sums them per tile now: 4.16e-7.)"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import reference_np as R
from papc_amd import _lib, smallm
from papc_amd import compact as C
from papc_amd import functional as F
from papc_amd.mlp import StackSpec, shared_mlp_max
from papc_amd.synthetic import make_clouds, make_start_idx
from tests import torch_ref
from tests.util import assert_close, fps_lattice, kernel_decisions, seeded_weights

pytestmark = pytest.mark.gpu

KNOBS = ("PAPC_STREAM", "PAPC_STREAM_MINTILES", "PAPC_STREAM_ASM", "PAPC_PARTS", "PAPC_LG_PARTS", "PAPC_LG_LISTS", "PAPC_GEMM_MINWG",
         "PAPC_GEMM_KB", "PAPC_GEMM_WAVES", "PAPC_FPS_THREADS", "PAPC_FPS_THREADS_SMALL")


def _knob_get(name):
    v = ctypes.c_int(0)
    _lib.check(_lib.load().papc_knob_get(name.encode(), ctypes.byref(v)), "papc_knob_get")
    return v.value


def _knob(name, value):
    _lib.check(_lib.load().papc_knob_set(name.encode(), int(value)), "papc_knob_set")


@pytest.fixture
def knobs():
    old = {n: _knob_get(n) for n in KNOBS}
    yield old
    for n, v in old.items():
        _knob(n, v)


# ---- (a) shared-MLP stacks ------------------------------------------------------------------------------------------------------------

PLAIN = {   # name: (G, K, channels)
    "P1": (32, 32, [64, 64, 128]),      # 8 row tiles; fused group max K = 32 once the 128-wide tile is allowed
    "P2": (16, 64, [128, 128, 256]),    # fused group max K = 64; two 128-column tiles
    "P3": (8, 128, [32, 64, 128]),      # the K = 128 exchange through LDS
    "P4": (37, 24, [64, 96, 128]),      # M = 888: 7 tiles, the last of 120 rows; ragged Cout; no fused max
    "P5": (37, 24, [13, 40, 24]),       # Cin % 4 != 0: the non-vector generic kernels
}
GROUPED = {  # name: (B, N, S, K, D, mlp, xyz_first) -- from test_gpu_mlp.py::test_stack_backward_vs_torch
    "G1": (2, 512, 64, 32, 0, [64, 64, 128], True),
    "G2": (2, 256, 32, 16, 12, [32, 40, 24], False),     # gathered first layer and the scatter dX
    "G3": (2, 256, 32, 16, 128, [128, 64], True),        # the gather-add first layer
}
_C = {"PAPC_STREAM": 0, "PAPC_GEMM_MINWG": 1, "PAPC_GEMM_KB": 1}
SETTINGS = {
    "A": {"PAPC_STREAM": 0, "PAPC_PARTS": 1},                       # one workgroup walks every tile
    "B": {"PAPC_STREAM": 0, "PAPC_PARTS": 3},                       # uneven split (3/3/2 or 3/2/2 tiles), the tail tile inside the loop
    "C": dict(_C),                                                  # the 128 x 128 tile with 16-deep stages
    "D": dict(_C, PAPC_GEMM_WAVES=4),                               # its 4-wave form
    "E": {"PAPC_STREAM": 0, "PAPC_GEMM_MINWG": 1, "PAPC_GEMM_KB": 2},   # 32-deep stages on the wide tile
    # narrowest tiles everywhere, the max unfused (papc_mlp_gemm_gmax_ok follows the knob).  At <= 8 row tiles the default rule lands on
    # the same 32-column configuration: this setting pins it whatever the default threshold becomes
    "F": {"PAPC_STREAM": 0, "PAPC_GEMM_MINWG": 4096},
    "G": dict(_C, PAPC_PARTS=3),                                    # the benchmark's flavour and its multi-tile loop together
    # the row-streaming kernels on a capped grid (P1-P4: the shapes they accept)
    "H": {"PAPC_STREAM": 1, "PAPC_STREAM_MINTILES": 1, "PAPC_PARTS": 1},
    "I1": {"PAPC_STREAM": 1, "PAPC_STREAM_MINTILES": 1, "PAPC_PARTS": 3, "PAPC_STREAM_ASM": 1},
    "I0": {"PAPC_STREAM": 1, "PAPC_STREAM_MINTILES": 1, "PAPC_PARTS": 3, "PAPC_STREAM_ASM": 0},
}
TILED, STREAMED = ("A", "B", "C", "D", "E", "F", "G"), ("H", "I1", "I0")
NAMES = ["w", "b", "gamma", "beta"]


def _finish(out, params, gin, gout, rows64, K):
    """backward + the float64 reference on the kernel's own decisions; everything a comparison needs, on the host"""
    L = len(params) // 4
    argmax, alive, masks = kernel_decisions(out)
    out.backward(gout)
    torch.cuda.synchronize()
    p64 = [p.detach().double().requires_grad_(True) for p in params]
    g64 = gin.detach().double().requires_grad_(True) if gin is not None else None
    ref, stats = torch_ref.stack_routed(rows64(g64), [tuple(p64[4 * l:4 * l + 4]) for l in range(L)], K, 1e-5, argmax, alive, masks)
    ref.backward(gout.double())
    cpu = lambda t: t.detach().cpu().numpy()        # noqa: E731
    return {"out": cpu(out), "grads": [cpu(p.grad) for p in params], "gin": cpu(gin.grad) if gin is not None else None,
            "ref_out": cpu(ref), "ref_grads": [cpu(p.grad) for p in p64], "ref_gin": cpu(g64.grad) if g64 is not None else None,
            "flips": stats, "L": L}


def _run_plain(dev, G, K, chans, seed=3):
    """the harness of test_gpu_stream.py::_run (plain rows [M, chans[0]] -> max over groups of K), under whatever knobs are set"""
    M = G * K
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.normal(size=(M, chans[0])).astype(np.float32)).to(dev).requires_grad_(True)
    ws = seeded_weights(chans, seed + 1)
    params = [torch.from_numpy(a).to(dev).requires_grad_(True) for tup in ws for a in tup]
    gout = torch.from_numpy(rng.normal(size=(G, chans[-1])).astype(np.float32)).to(dev)
    spec = StackSpec(1, M, G, K, chans[0] - 3, True)
    xyz = torch.zeros(1, 1, 3, device=dev)
    # (P3 -- groups of exactly 128 rows -- would take the planes path, smallm.hip, which none of these knobs reaches: row kernels for all)
    old = smallm.ENABLED
    smallm.ENABLED = False
    try:
        out = shared_mlp_max(spec, None, xyz, xyz, None, None, params, x_rows=x)
    finally:
        smallm.ENABLED = old
    assert not out.grad_fn.planes
    res = _finish(out, params, x, gout, lambda x64: x64, K)
    res["gmax"] = bool(out.grad_fn.plan.gmax)        # (whether the library planned the fused group max for this run)
    return res


def _grouping(dev, B, N, S, K):
    x = make_clouds(B, N, 31 + N)
    xyz = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).to(dev)
    st = torch.from_numpy(make_start_idx(B, N, 1)).to(dev)
    _, new_xyz = F._fps_raw(xyz, S, st)
    idx = F._ball_query_raw([0.3], [K], xyz, new_xyz)[0]
    return xyz, new_xyz, idx


def _run_grouped(dev, B, N, S, K, D, mlp, xyz_first, seed=40, grouping=None, lists=False):
    """the harness of test_gpu_mlp.py::test_stack_backward_vs_torch, under whatever knobs are set"""
    xyz, new_xyz, idx = grouping if grouping is not None else _grouping(dev, B, N, S, K)
    rng = np.random.default_rng(8)
    feats = torch.from_numpy(rng.normal(size=(B, N, D)).astype(np.float32)).to(dev).requires_grad_(True) if D else None
    ws = seeded_weights([D + 3] + mlp, seed)
    params = [torch.from_numpy(a).to(dev).requires_grad_(True) for tup in ws for a in tup]
    spec = StackSpec(B, N, S, K, D, xyz_first)
    if lists:
        spec.plists = C.point_lists(xyz, new_xyz, idx, None)
    out = shared_mlp_max(spec, None, xyz, new_xyz, feats, idx, params)
    gout = torch.from_numpy(rng.normal(size=tuple(out.shape)).astype(np.float32)).to(dev)
    rows64 = lambda f64: torch_ref.group(xyz.double(), new_xyz.double(), f64, idx, xyz_first).reshape(B * S * K, D + 3)     # noqa: E731
    return _finish(out, params, feats, gout, rows64, K)


def _check(run, base, what):
    """both sets of bars; returns the worst (f64 forward, f64 gradient, cross forward, cross gradient)"""
    print("decisions that differ from float64's own:", run["flips"])
    worst = [0.0, 0.0, 0.0, 0.0]
    worst[0] = assert_close(run["out"], run["ref_out"], 1e-5, what + " forward vs f64")
    for l in range(run["L"]):
        for j in range(4):
            got, want = run["grads"][4 * l + j], run["ref_grads"][4 * l + j]
            if j == 1:
                # conv bias feeds a train-mode BN: its true gradient is exactly zero; both sides hold rounding noise
                scale = float(np.abs(run["ref_grads"][4 * l]).max())
                assert float(np.abs(got).max()) <= 1e-4 * scale, "%s db layer %d not ~0" % (what, l)
                continue
            worst[1] = max(worst[1], assert_close(got, want, 2e-4, "%s d%s layer %d vs f64" % (what, NAMES[j], l)))
    if run["gin"] is not None:
        worst[1] = max(worst[1], assert_close(run["gin"], run["ref_gin"], 2e-4, what + " input gradient vs f64"))
    # the default geometry on the same input: the same products, another order of the BatchNorm partial sums (gemm_kernel sums a tile's
    # statistics from zero before adding them to the workgroup's running pair, so the order matters little however many tiles it walks)
    worst[2] = assert_close(run["out"], base["out"], 2e-6, what + " forward vs default knobs")
    for l in range(run["L"]):
        for j in (0, 2, 3):
            worst[3] = max(worst[3], assert_close(run["grads"][4 * l + j], base["grads"][4 * l + j], 2e-5,
                                                  "%s d%s layer %d vs default knobs" % (what, NAMES[j], l)))
    if run["gin"] is not None:
        worst[3] = max(worst[3], assert_close(run["gin"], base["gin"], 2e-5, what + " input gradient vs default knobs"))
    print("[geometry] %s: vs f64 forward %.2e gradients %.2e | vs default forward %.2e gradients %.2e" % (what, *worst))
    return worst


_BASE = {}     # shape name -> the run at default knobs (computed once, shared by the settings, never modified)


def _baseline(dev, knobs, shape):
    if shape not in _BASE:
        assert all(_knob_get(n) == v for n, v in knobs.items())      # nothing applied yet: the defaults
        _BASE[shape] = _run_plain(dev, *PLAIN[shape]) if shape in PLAIN else _run_grouped(dev, *GROUPED[shape])
    return _BASE[shape]


def _apply(setting):
    for n, v in SETTINGS[setting].items():
        _knob(n, v)


# (H and I are P1-P4's: the row-streaming kernels take no 13-channel input.  No (shape, setting) pair of A-G is left out.)
@pytest.mark.parametrize("shape,setting", [(s, t) for s in sorted(PLAIN) for t in TILED + (STREAMED if s != "P5" else ())])
def test_plain_stack_under_scaled_geometry(dev, knobs, shape, setting):
    G, K, chans = PLAIN[shape]
    base = _baseline(dev, knobs, shape)
    _apply(setting)                  # held from before the forward until after backward() and its synchronize (_finish)
    lib = _lib.load()
    want_parts = min((G * K + 127) // 128, SETTINGS[setting].get("PAPC_PARTS", knobs["PAPC_PARTS"]))
    assert lib.papc_mlp_gemm_parts(G * K) == want_parts
    if setting in ("C", "D", "E", "G"):     # the 128-wide tile is allowed at 7 or 8 row tiles: so is the fused max, where its other rules hold
        assert lib.papc_mlp_gemm_gmax_ok(G * K, chans[-1], K) == (1 if shape in ("P1", "P2", "P3") else 0)
    if setting in ("A", "B", "F"):
        assert lib.papc_mlp_gemm_gmax_ok(G * K, chans[-1], K) == 0
    run = _run_plain(dev, G, K, chans)
    assert run["gmax"] == (setting in ("C", "D", "E", "G") and shape in ("P1", "P2", "P3"))
    _check(run, base, "%s/%s" % (shape, setting))


@pytest.mark.parametrize("setting", TILED)
@pytest.mark.parametrize("shape", sorted(GROUPED))
def test_grouped_stack_under_scaled_geometry(dev, knobs, shape, setting):
    base = _baseline(dev, knobs, shape)
    _apply(setting)
    run = _run_grouped(dev, *GROUPED[shape])
    _check(run, base, "%s/%s" % (shape, setting))


# ---- (b) gather-add partition -----------------------------------------------------------------------------------------------------------

def _cut_grouping(dev):
    """G3's grouping with the groups that the workgroup boundaries cut made of ONE repeated index: rows_per_wg = 342 (PAPC_LG_PARTS=3) cuts
    groups 21 and 42, rows_per_wg = 205 (=5) cuts groups 12, 25, 38, 51 (16 rows each) -- all but their first row are padding duplicates,
    so the pending duplicate sum of lingather_bwd_kernel is non-empty at every boundary"""
    B, N, S, K = GROUPED["G3"][:4]
    xyz, new_xyz, idx = _grouping(dev, B, N, S, K)
    idx = idx.clone()
    flat = idx.view(B * S, K)
    for g in (12, 21, 25, 38, 42, 51):
        flat[g, :] = flat[g, 0].clone()
    return xyz, new_xyz, idx


@pytest.mark.parametrize("lists", [0, 1])
@pytest.mark.parametrize("lg_parts", [1, 3, 5])
def test_gather_add_partition_cuts_groups(dev, knobs, lg_parts, lists):
    B, N, S, K, D, mlp, xyz_first = GROUPED["G3"]
    M = B * S * K
    lib = _lib.load()
    if "cut" not in _BASE:
        assert all(_knob_get(n) == v for n, v in knobs.items())
        grouping = _cut_grouping(dev)
        _BASE["cut"] = (grouping, _run_grouped(dev, *GROUPED["G3"], grouping=grouping, lists=True))     # default knobs: the list backward
    grouping, base = _BASE["cut"]
    assert lib.papc_lingather_parts(M) == 8
    _knob("PAPC_LG_PARTS", lg_parts)
    _knob("PAPC_LG_LISTS", lists)
    parts = lib.papc_lingather_parts(M)
    assert parts == lg_parts and (M + parts - 1) // parts == {1: 1024, 3: 342, 5: 205}[lg_parts]
    run = _run_grouped(dev, B, N, S, K, D, mlp, xyz_first, grouping=grouping, lists=bool(lists))
    _check(run, base, "G3cut/LG_PARTS=%d,LISTS=%d" % (lg_parts, lists))


# ---- (c) FPS geometries -------------------------------------------------------------------------------------------------------------------

_LATTICE = fps_lattice(2, 26)


def _fps_inputs(B, N):
    """(name, xyz [B, N, 3], start [B], init_dist)"""
    x = make_clouds(B, N, 11 + N)
    yield "clouds", np.ascontiguousarray(x.transpose(0, 2, 1)), make_start_idx(B, N, 5), 1.0
    lat = np.ascontiguousarray(_LATTICE[:, :N])
    st = np.random.default_rng(N).integers(0, N, size=B).astype(np.int64)
    for init in (1e10, 1.0):
        yield "lattice init %g" % init, lat, st, init


@pytest.mark.parametrize("PPT", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("T", [64, 128, 256, 512, 1024])
def test_fps_every_geometry_index_exact(dev, knobs, T, PPT):
    """fps_kernel<T, PPT> for all 25 instantiations (the default rule reaches about ten), index-exact against the oracle on random clouds
    and on the lattice prefix whose squared distances are exact and tie in most iterations."""
    B = 2
    _knob("PAPC_FPS_THREADS", T)
    _knob("PAPC_FPS_THREADS_SMALL", T)
    sizes = (max(1, T // 2 + 1), T - 3, T) if PPT == 1 else (T * PPT // 2 + 1, T * PPT - 3, T * PPT)
    for N in sizes:
        # the rule of papc_fps_f32 (sampling.hip): T from the knob, points per thread doubled until they cover N; T itself doubles only past 16
        t, ppt = T, 1
        while t * ppt < N:
            ppt *= 2
        assert (t, ppt) == (T, PPT) and ppt <= 16 and N <= 16384
        npoint = min(N, 32)
        for name, xyz, st, init in _fps_inputs(B, N):
            ref = R.farthest_point_sample(xyz, npoint, st, init).astype(np.int64)
            for planar in (False, True):
                t_xyz = torch.from_numpy(xyz).to(dev)
                if planar:
                    t_xyz = t_xyz.transpose(1, 2).contiguous().transpose(1, 2)
                    assert t_xyz.stride() == (3 * N, 1, N)
                got = F.farthest_point_sample(t_xyz, npoint, torch.from_numpy(st).to(dev), init_dist=init)
                assert np.array_equal(got.cpu().numpy(), ref), (T, PPT, N, name, "planar" if planar else "strided")
