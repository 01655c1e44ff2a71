"""The compacted and point-list paths of a gather-add stack on ENGINEERED groupings (tests/grouping_cases.py), at test-sized shapes.

SA2 of the benchmark's step runs on the compacted rows (csrc/compact.hip) and takes its gather-add backward over point lists
(csrc/lingather.hip, papc_lingather_bwd_pp_f32).  papc_mlp_compact_ok refuses a stack below PAPC_STREAM_MINTILES tiles, so the suite ran
that code only at B = 8 and 16 on FPS + ball-query lists of make_clouds -- one kind of list.  Here the threshold is scaled down
(PAPC_STREAM_MINTILES=1 through papc_knob_set) and the lists are built by hand: B = 2, S = 16, K in {8, 16, 64}, N = 64 or 96, D = 16, stacks
[D + 3, 128, 128, 256] and [D + 3, 128, 256]; with PAPC_PARTS=3 / PAPC_LG_PARTS=3 workgroups walk several row tiles and cut groups.
feats and xyz are views into NaN-guarded buffers (one spare NaN row before and after the real rows): a loader that follows an out-of-range index
reads a NaN inside the allocation and the output is not finite.

Bars (tests/test_gpu_compact.py): against float64 torch autograd on the PADDED rows routed through the kernel's own decisions
(torch_ref.stack_routed, util.kernel_decisions) forward 1e-5, gradients 2e-4; compacted against padded and lists against atomics 2e-6 / 2e-5; two
runs of a list path bit-identical; plan and list tensors bit for bit the numpy models (grouping_cases.plan_model, test_gpu_compact._numpy_lists).

What each case is the smallest instance of, and what fails if the kernel is wrong:
  E1 singletons -- a group that is ONE row plus multiplicity.  compact_fill_kernel's wrow[s] = 1 + K - n carries 57 of 64 rows at K = 64: a
     lost weight (lingather_fwd_kernel's s_wq, gemm rows' wrow) moves every BatchNorm mean.  K = 8: coef 0, the plan must change nothing.
  E2 full -- the plan forced on where nothing is a copy: every weight 1, physical rows == capacity; a kernel that sizes a loop from the row
     count rounded differently than the capacity reads past the last tile or drops it.
  E3 count sweep -- cnt = 1 .. K: no pad rows (cnt % 8 == 0), seven pad rows (cnt % 8 == 1), cnt == K.  compact_count_kernel's (n + 8) & ~7 and
     the pad rows' weight 1 (they are COPIES: counted once each, K - n left on the first row).
  E4 row-count boundaries -- a: the total is a multiple of 128 (compact_scan_kernel's (total + 127) & ~127 must not add a tile; the last group
     has no pad row); b: total = 8 mod 128, singleton last: 120 tail rows in one group, first-row weight 1 + 16 - 128 = -111.  seg_max_kernel
     stops at start[G] (the tail is outside), the list builder's row_of(G) = rows[0] takes the tail into the last group's lists.
  E5 hub and orphans -- a: one point in all S groups as a non-first neighbour (a list of S weight-1 entries, one wave in
     lingather_bwd_pp_kernel's base loop); b: the same point first everywhere (the padded builder's ONE weighted copy entry per group,
     `ncopy`; the compacted wrow on every entry).  Half the points are in no group: prange empty, dfeats rows exactly 0.0 (the list kernels
     WRITE G, the atomic one relies on the zero fill).
  E6 interior repeats -- a non-first index twice (point_lists_kernel's lane-sweep ranking, `clash`) and the first index mid-list (a copy for
     the padded builder and for lingather_bwd_kernel's s_dup, wherever it sits).  The compacted plan does NOT take such lists (it keeps a
     list's first rows by position: include/papc_hip.h, papc_compact_plan_f32; grouping_cases.plan_model shows the lost neighbour), so E6 runs
     on the padded and list paths only.
  E7 no-hit rows -- N and -1 among the non-first entries and a group that is entirely N: zero INPUT rows (y = bias) that count in the
     statistics and the max and send nothing to dfeats / dW_x.  Guards: lg_row (lingather.hip), point_lists_kernel's j < 0 || j >= N,
     make_row (mlp_loaders.h; D = 12, the gathered first layer and its scatter dX in gemm_kernel), xyz_group_kernel (xyz1.hip; D = 0).
  E8 duplicated cloud -- through PointNetSetAbstraction (FPS and ball query on points that tie exactly), compact=True and compact=None.
Negative controls: one first-row weight set to 1 (E3), one list entry's weight set to 0 (E5b) -- the float64 comparison must then fail.

Measured on the MI355X, worst over the file (forward / gradients): 5.83e-7 / 3.34e-6 against float64, 5.85e-7 / 3.34e-6 compacted against padded,
0 / 4.77e-6 lists against atomics (the forward does not depend on the backward's form).  The controls: forward 2.32e-2 against float64 with one
first-row weight of 9 set to 1 (bar 1e-5), first-layer dW 5.75e-2 with one copy entry's weight set to 0 (bar 2e-4)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import reference_np as R
from papc_amd import _lib
from papc_amd import compact as C
from papc_amd import mlp
from papc_amd.layers import PointNetSetAbstraction
from papc_amd.mlp import StackSpec, shared_mlp_max
from tests import grouping_cases as GC
from tests import torch_ref
from tests.test_gpu_compact import _collapse_copies, _numpy_lists
from tests.util import assert_close, kernel_decisions, seeded_weights

pytestmark = pytest.mark.gpu

KNOBS = ("PAPC_STREAM_MINTILES", "PAPC_PARTS", "PAPC_LG_PARTS", "PAPC_LG_LISTS", "PAPC_LG_PP")
B, S, D = GC.B, GC.S, 16
L3, L2 = [128, 128, 256], [128, 256]
NAMES = ["w", "b", "gamma", "beta"]
# name: (compacted, point lists handed over, PAPC_LG_LISTS, PAPC_LG_PP)
PATHS = {
    "padded/atomic": (False, True, 0, 1),         # (lists handed over and refused by the knob: the float-atomic kernel)
    "padded/lists-pp": (False, True, 1, 1),
    "padded/lists-y": (False, True, 1, 0),
    "compact/atomic": (True, False, 1, 1),        # compacted without lists
    "compact/lists-pp": (True, True, 1, 1),
    "compact/lists-y": (True, True, 1, 0),
}
CASES = {
    "E1k8": lambda: GC.e1_singletons(8), "E1k64": lambda: GC.e1_singletons(64), "E2": GC.e2_full, "E3": GC.e3_count_sweep,
    "E3k64": lambda: GC.e3_count_sweep(64),
    "E4a": lambda: GC.e4_row_boundary("a"), "E4b": lambda: GC.e4_row_boundary("b"), "E5a": lambda: GC.e5_hub_orphans("a"),
    "E5b": lambda: GC.e5_hub_orphans("b"), "E6": GC.e6_interior_repeats, "E7": GC.e7_no_hit,
}
WORST = {"f64 forward": 0.0, "f64 gradients": 0.0, "compacted vs padded forward": 0.0, "compacted vs padded gradients": 0.0,
         "lists vs atomics forward": 0.0, "lists vs atomics gradients": 0.0}


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


def _geometry(geom):
    _knob("PAPC_STREAM_MINTILES", 1)
    if geom == "parts3":
        _knob("PAPC_PARTS", 3)
        _knob("PAPC_LG_PARTS", 3)


# ---- inputs: built once per (case, D), never modified ---------------------------------------------------------------------------------------

_INPUTS = {}


def _inputs(dev, name, case=None, Dd=D):
    key = (name, Dd)
    if key not in _INPUTS:
        case = case if case is not None else CASES[name]()
        N, K = case["N"], case["K"]
        xyz, feats, new_xyz = GC.materialise(case, Dd)
        xb = torch.full((B, N + 2, 3), float("nan"), device=dev)              # a NaN row before and after every cloud's points
        xb[:, 1:N + 1] = torch.from_numpy(xyz).to(dev)
        fv = None
        if Dd:
            fb = torch.full((B * N + 2, Dd), float("nan"), device=dev)        # ... and around the (contiguous) feature rows
            fb[1:-1] = torch.from_numpy(feats.reshape(B * N, Dd)).to(dev)
            fv = fb[1:-1].view(B, N, Dd)
            assert fv.is_contiguous() and fv.data_ptr() % 16 == 0
        ii = case["idx"]
        used = np.zeros((B, N), bool)
        for b in range(B):
            v = ii[b][(ii[b] >= 0) & (ii[b] < N)]
            used[b, v] = True
        _INPUTS[key] = dict(name=case["name"], N=N, K=K, D=Dd, ii=ii, idx=torch.from_numpy(ii).to(dev), xyz=xb[:, 1:N + 1], feats=fv,
                            new_xyz=torch.from_numpy(new_xyz).to(dev), used=used, xyz_np=xyz, new_np=new_xyz)
    return _INPUTS[key]


def _rows64(inp, f64, xyz_first):
    """the float64 reference's grouped rows [M, D + 3]: the same gather, with a ZERO row wherever the index is outside [0, N)"""
    N = inp["N"]
    idx = inp["idx"].long()
    valid = (idx >= 0) & (idx < N)
    safe = idx.clamp(0, N - 1).int()
    rows = torch_ref.group(inp["xyz"].double(), inp["new_xyz"].double(), f64, safe, xyz_first)
    rows = torch.where(valid[..., None], rows, torch.zeros_like(rows))
    return rows.reshape(B * S * inp["K"], inp["D"] + 3)


def _group_src(inp, cp, pl, keep):
    g = _lib.GroupSrc()
    xyz = inp["xyz"]
    g.xyz, g.sb, g.sn, g.sc = xyz.data_ptr(), xyz.stride(0), xyz.stride(1), xyz.stride(2)
    g.new_xyz, g.idx = inp["new_xyz"].data_ptr(), inp["idx"].data_ptr()
    g.N, g.S, g.K, g.D, g.xyz_first = inp["N"], S, inp["K"], inp["D"], 1
    if cp is not None:
        g.cidx, g.seg_grp, g.rows_dev, g.wstat = cp.cidx.data_ptr(), cp.seg_grp.data_ptr(), cp.rows.data_ptr(), cp.wrow.data_ptr()
    if pl is not None:
        src = _lib.PointLists(pl.prange.data_ptr(), pl.prow.data_ptr(), pl.pmeta.data_ptr(), int(pl.compact), pl.pmom.data_ptr())
        keep.append(src)
        g.plists = ctypes.addressof(src)
    return g


def _run(dev, inp, widths, compact, lists, xyz_first=True, corrupt=None, seed=70, f64=True):
    """one forward + backward under whatever knobs are set -> everything a comparison needs, on the host"""
    lib = _lib.load()
    N, K, Dd = inp["N"], inp["K"], inp["D"]
    feats = inp["feats"].detach().requires_grad_(True) if Dd else None
    ws = seeded_weights([Dd + 3] + widths, seed)
    params = [torch.from_numpy(a).to(dev).requires_grad_(True) for tup in ws for a in tup]
    spec = StackSpec(B, N, S, K, Dd, xyz_first)
    cp = C.plan(inp["idx"]) if compact else None
    pl = C.point_lists(inp["xyz"], inp["new_xyz"], inp["idx"], cp) if lists else None
    if corrupt is not None:
        torch.cuda.synchronize()
        corrupt(cp, pl)
    spec.compact, spec.plists = cp, pl
    out = shared_mlp_max(spec, None, inp["xyz"], inp["new_xyz"], feats, inp["idx"], params)
    node = out.grad_fn
    assert (node.compact is not None) == compact, "the compacted path was %staken" % ("not " if compact else "")
    flags = None
    if lists:           # what the library's own rule says the gather-add backward will do with these lists (no silent fallback)
        keep = []
        g = _group_src(inp, cp, pl, keep)
        flags = (lib.papc_lingather_bwd_lists_ok(ctypes.byref(g), widths[0]), lib.papc_lingather_bwd_pp_ok(ctypes.byref(g), B, widths[0]))
    L = len(widths)
    argmax, alive, masks = kernel_decisions(out)
    gout = torch.from_numpy(np.random.default_rng(7).normal(size=tuple(out.shape)).astype(np.float32)).to(dev)
    out.backward(gout)
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu().numpy()        # noqa: E731
    res = {"out": cpu(out), "grads": [cpu(p.grad) for p in params], "gin": cpu(feats.grad) if Dd else None, "L": L, "cp": cp, "pl": pl,
           "flags": flags, "node": node}
    assert np.isfinite(res["out"]).all() and all(np.isfinite(a).all() for a in res["grads"]), "non-finite output: a loader followed an index"
    assert res["gin"] is None or np.isfinite(res["gin"]).all()
    if f64:
        p64 = [p.detach().double().requires_grad_(True) for p in params]
        g64 = feats.detach().double().requires_grad_(True) if Dd else None
        ref, stats = torch_ref.stack_routed(_rows64(inp, g64, xyz_first), [tuple(p64[4 * l:4 * l + 4]) for l in range(L)], K, 1e-5, argmax, alive, masks)
        ref.backward(gout.double())
        res.update(ref_out=cpu(ref), ref_grads=[cpu(p.grad) for p in p64], ref_gin=cpu(g64.grad) if Dd else None, flips=stats)
    return res


def _vs_f64(run, what):
    print("decisions that differ from float64's own:", run["flips"])
    WORST["f64 forward"] = max(WORST["f64 forward"], assert_close(run["out"], run["ref_out"], 1e-5, what + " forward vs f64"))
    w = 0.0
    for l in range(run["L"]):
        for j in range(4):
            got, want = run["grads"][4 * l + j], run["ref_grads"][4 * l + j]
            if j == 1:      # conv bias under a train-mode BN: its true gradient is exactly zero; both sides hold rounding noise
                assert float(np.abs(got).max()) <= 1e-4 * float(np.abs(run["ref_grads"][4 * l]).max()), "%s db layer %d not ~0" % (what, l)
                continue
            w = max(w, assert_close(got, want, 2e-4, "%s d%s layer %d vs f64" % (what, NAMES[j], l)))
    if run["gin"] is not None:
        w = max(w, assert_close(run["gin"], run["ref_gin"], 2e-4, what + " dfeats vs f64"))
    WORST["f64 gradients"] = max(WORST["f64 gradients"], w)


def _cross(run, base, kind, what):
    """``kind``: "compacted vs padded" or "lists vs atomics" -- forward 2e-6, gradients 2e-5"""
    f = assert_close(run["out"], base["out"], 2e-6, "%s: %s forward" % (what, kind))
    w = 0.0
    for l in range(run["L"]):
        for j in (0, 2, 3):
            w = max(w, assert_close(run["grads"][4 * l + j], base["grads"][4 * l + j], 2e-5, "%s: %s d%s layer %d" % (what, kind, NAMES[j], l)))
    if run["gin"] is not None:
        w = max(w, assert_close(run["gin"], base["gin"], 2e-5, "%s: %s dfeats" % (what, kind)))
    WORST[kind + " forward"] = max(WORST[kind + " forward"], f)
    WORST[kind + " gradients"] = max(WORST[kind + " gradients"], w)


def _same_bits(a, b, what):
    assert np.array_equal(a["out"], b["out"]), what + ": forward differs between two runs"
    for i, (x, y) in enumerate(zip(a["grads"], b["grads"])):
        assert np.array_equal(x, y), "%s: gradient %d differs between two runs" % (what, i)
    assert np.array_equal(a["gin"], b["gin"]), what + ": dfeats differs between two runs"


def _report():
    print("[groupings] worst so far: " + ", ".join("%s %.2e" % kv for kv in WORST.items()))


# ---- the plan and the lists against their numpy models ---------------------------------------------------------------------------------------

def _check_plan(cp, inp):
    m = GC.plan_model(inp["ii"].reshape(B * S, inp["K"]))
    rows = m["rows"]
    assert cp.rows.cpu().tolist() == [rows, m["total"]]
    assert np.array_equal(cp.start.cpu().numpy(), m["start"])
    assert np.array_equal(cp.cidx.cpu().numpy()[:rows], m["cidx"]) and np.array_equal(cp.wrow.cpu().numpy()[:rows], m["wrow"])
    assert np.array_equal(cp.seg_grp.cpu().numpy()[:rows // 8], m["seg"]) and np.array_equal(cp.coef.cpu().numpy(), m["coef"])
    return m


def _check_lists(pl, cp, inp):
    N, K = inp["N"], inp["K"]
    if cp is not None:
        rows = int(cp.rows[0])
        rows_pt = cp.cidx.cpu().numpy()[:rows].astype(np.int64)
        rows_grp = np.repeat(cp.seg_grp.cpu().numpy()[:rows // 8], 8).astype(np.int64)
        w = cp.wrow.cpu().numpy()[:rows]
    else:
        rows_pt, rows_grp, w = _collapse_copies(inp["ii"], N)
    prange, key, rws, meta = _numpy_lists(B, N, S, K, inp["xyz_np"], inp["new_np"], rows_pt, rows_grp, w)
    assert np.array_equal(pl.prange.cpu().numpy(), prange)
    prow, pmeta = pl.prow.cpu().numpy(), pl.pmeta.cpu().numpy()
    seen = 0
    for q in range(B * N):
        a, b_ = prange[q]
        want = rws[key == q] if b_ > a else np.zeros(0, np.int64)
        assert np.array_equal(prow[a:b_], want), q
        for e, r in zip(range(a, b_), want):
            assert tuple(pmeta[e]) == tuple(np.float32(v) for v in meta[int(r)]), (q, r)
        seen += b_ - a
        if not inp["used"].reshape(-1)[q]:
            assert a == b_, "a point no group gathered has a list"
    assert seen == int(((rows_pt >= 0) & (rows_pt < N)).sum()) and pl.compact == (cp is not None)
    mom = pl.pmom.cpu().numpy()
    want = np.zeros((B * N, 10))
    for q in range(B * N):
        e = pmeta[prange[q, 0]:prange[q, 1]].astype(np.float64)
        wq, dq = e[:, 3], e[:, :3]
        m2 = np.einsum("e,es,et->st", wq, dq, dq)
        want[q] = [wq.sum(), *(wq[:, None] * dq).sum(0), m2[0, 0], m2[0, 1], m2[0, 2], m2[1, 1], m2[1, 2], m2[2, 2]]
    assert not mom[:, 10:].any() and np.abs(mom[:, :10] - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


# ---- E1 - E7 through every path ---------------------------------------------------------------------------------------------------------------

def _all_paths(dev, name, widths, geom, models):
    inp = _inputs(dev, name)
    _geometry(geom)
    runs = {}
    for path, (compact, lists, k_lists, k_pp) in PATHS.items():
        if compact and name == "E6":
            continue                 # (the plan does not take a copy of the first entry ahead of another entry: papc_hip.h)
        _knob("PAPC_LG_LISTS", k_lists)
        _knob("PAPC_LG_PP", k_pp)
        what = "%s/%s/%s/%d layers" % (name, path, geom, len(widths))
        run = runs[path] = _run(dev, inp, widths, compact, lists)
        assert run["node"].lin0, "the gather-add first layer was not taken"
        if lists:
            assert run["flags"] == (k_lists, k_lists and k_pp), "%s: the library would not take this list path: %r" % (what, run["flags"])
        _vs_f64(run, what)
        if lists and k_lists:
            _same_bits(run, _run(dev, inp, widths, compact, lists, f64=False), what)
        if not inp["used"].all():    # a point no group gathered: zero gradient, exactly (the list kernels WRITE those rows of G)
            assert not run["gin"][~inp["used"]].any(), what + ": a point in no group has a gradient"
        if models and compact:
            _check_plan(run["cp"], inp)
        if models and lists:
            _check_lists(run["pl"], run["cp"], inp)
    for path, run in runs.items():
        layout, bwd = path.split("/")
        if layout == "compact":
            _cross(run, runs["padded/" + bwd], "compacted vs padded", "%s/%s/%s" % (name, bwd, geom))
        if bwd != "atomic":
            _cross(run, runs[layout + "/atomic"], "lists vs atomics", "%s/%s/%s" % (name, path, geom))
    _report()
    return runs


@pytest.mark.parametrize("geom", ["default", "parts3"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_grouping_through_every_path(dev, knobs, name, geom):
    runs = _all_paths(dev, name, L3, geom, models=(geom == "default"))
    if name == "E1k8":      # coef 0: the plan compacts nothing -- every weight 1, as many rows as the padded stack
        cp = runs["compact/atomic"]["cp"]
        assert not cp.coef.cpu().numpy().any() and cp.rows.cpu().tolist() == [B * S * 8, B * S * 8]
    if name == "E2":
        assert runs["compact/atomic"]["cp"].fraction() == 1.0
    if name == "E4b":
        assert float(runs["compact/atomic"]["cp"].coef[-1]) == 16 - 128


@pytest.mark.parametrize("name", ["E3", "E4b", "E7"])
def test_two_layer_stack_through_every_path(dev, knobs, name):
    """[D + 3, 128, 256]: the gather-add layer feeds the max layer directly -- the dX launch that stores the masked dz is the max layer's"""
    _all_paths(dev, name, L2, "parts3", models=False)


def test_unweighted_statistics_with_correction_launches(dev, knobs, monkeypatch):
    """PAPC_WSTATS=0 on E3: the unweighted sums + papc_bn_stats_corr_f32 (coef[g] y[start[g]]) against the producers' weighted sums"""
    inp = _inputs(dev, "E3")
    _geometry("parts3")
    base = _run(dev, inp, L3, True, True)
    monkeypatch.setenv("PAPC_WSTATS", "0")
    run = _run(dev, inp, L3, True, True)
    assert run["flags"] == (1, 1)
    _vs_f64(run, "E3/PAPC_WSTATS=0")
    assert_close(run["out"], base["out"], 2e-6, "E3: correction launches vs weighted statistics, forward")
    for i, (a, b_) in enumerate(zip(run["grads"], base["grads"])):
        if i % 4 != 1:
            assert_close(a, b_, 2e-5, "E3: correction launches vs weighted statistics, gradient %d" % i)
    assert_close(run["gin"], base["gin"], 2e-5, "E3: correction launches vs weighted statistics, dfeats")
    _report()


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("name", ["E3", "E5a", "E5b"])
def test_library_and_python_orchestrations(dev, knobs, monkeypatch, name, compact):
    """papc_sa_mlp_fwd / _bwd against the launch sequence spelled out in Python (mlp._PY_ORCH), both on the float-atomic gather-add backward and
    the correction-launch statistics (the forms the Python sequence has): the same kernels in the same order -- the same BITS in the forward and in
    every gradient the float atomics do not reach (the first layer's dW and dfeats read G, the atomic row sums)."""
    inp = _inputs(dev, name)
    _geometry("parts3")
    _knob("PAPC_LG_LISTS", 0)
    monkeypatch.setenv("PAPC_WSTATS", "0")
    res = {}
    for py in (False, True):
        monkeypatch.setattr(mlp, "_PY_ORCH", py)
        res[py] = _run(dev, inp, L3, compact, False)
        assert ("Stack" in type(res[py]["node"]).__name__) == (not py)
        _vs_f64(res[py], "%s/%s/%s orchestration" % (name, "compact" if compact else "padded", "python" if py else "library"))
    a, b_ = res[False], res[True]
    assert np.array_equal(a["out"], b_["out"]), "forward differs"
    for i, (x, y) in enumerate(zip(a["grads"], b_["grads"])):
        if i == 0:
            assert float(np.abs(x - y).max()) <= 1e-5 * float(np.abs(x).max()), "first-layer dW differs beyond atomic-order noise"
        else:
            assert np.array_equal(x, y), "gradient %d differs" % i
    assert float(np.abs(a["gin"] - b_["gin"]).max()) <= 1e-5 * float(np.abs(a["gin"]).max())
    _report()


# ---- negative controls: the bars see a wrong multiplicity at these shapes ---------------------------------------------------------------------

# what "the comparison fails" means: a bar of _vs_f64 is missed, or the float64 reference finds the kernel's winner off its own group maximum
# (torch_ref.stack_routed) -- not any other assertion on the way (the controls' own preconditions, the finiteness check)
_SEEN = r"vs f64: (max|elementwise) rel err|a pinned winner is not within"


def test_a_wrong_first_row_weight_fails_the_float64_comparison(dev, knobs):
    inp = _inputs(dev, "E3")
    _geometry("default")
    g = 16                      # cnt = 1: the first row carries 1 + 16 - 8 = 9 of the group's 16 slots

    def corrupt(cp, pl):
        s = int(cp.start[g])
        assert float(cp.wrow[s]) == 9.0
        cp.wrow[s] = 1.0
    _vs_f64(_run(dev, inp, L3, True, False), "E3 control, plan intact")
    # the routed reference already refuses the corrupted run (its winners are off float64's group maxima); the FORWARD against float64's own
    # decisions says by how much: 8 of 512 rows missing from every layer's statistics
    p64 = [torch.from_numpy(a).to(dev).double() for tup in seeded_weights([D + 3] + L3, 70) for a in tup]
    want = torch_ref.stack_max(_rows64(inp, inp["feats"].double(), True), [tuple(p64[4 * l:4 * l + 4]) for l in range(3)], inp["K"], 1e-5).cpu().numpy()
    assert_close(_run(dev, inp, L3, True, False, f64=False)["out"], want, 1e-5, "E3 control, plan intact: forward vs f64 (its own decisions)")
    bad = _run(dev, inp, L3, True, False, corrupt=corrupt, f64=False)
    with pytest.raises(AssertionError, match=_SEEN) as err:
        assert_close(bad["out"], want, 1e-5, "E3 control, wrow[start[16]] = 1: forward vs f64")
    print("[groupings] E3 control:", str(err.value).splitlines()[0])
    with pytest.raises(AssertionError, match=_SEEN):
        _vs_f64(_run(dev, inp, L3, True, False, corrupt=corrupt), "E3 control, wrow[start[16]] = 1")


def test_a_wrong_list_entry_weight_fails_the_float64_comparison(dev, knobs):
    inp = _inputs(dev, "E5b")
    _geometry("default")

    def corrupt(cp, pl):
        e = int(pl.prange[GC.HUB, 0]) + 1          # the hub's second entry: group 0's copies of it, ONE entry of weight = their number
        assert float(pl.pmeta[e, 3]) >= 2.0
        pl.pmeta[e, 3] = 0.0
    ok = _run(dev, inp, L3, False, True)
    assert ok["flags"] == (1, 1)
    _vs_f64(ok, "E5b control, lists intact")
    with pytest.raises(AssertionError, match=_SEEN) as err:
        _vs_f64(_run(dev, inp, L3, False, True, corrupt=corrupt), "E5b control, pmeta[e, 3] = 0")
    print("[groupings] E5b control:", str(err.value).splitlines()[0])


# ---- E7 on the other first layers ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["xyz1", "gathered"])
def test_no_hit_rows_on_the_other_first_layers(dev, knobs, kind):
    """the out-of-range rule where the first layer is not the gather-add: coordinates only (D = 0, [3, 64, 64, 128], K = 32: xyz_group_kernel's
    ``ok``) and a gathered first layer (D = 12: make_row's ``valid``, fetch_a4, the slot loader of mlp_dw.hip, the scatter dX's j range test)"""
    _geometry("parts3")
    if kind == "xyz1":
        inp = _inputs(dev, "E7k32", GC.e7_no_hit(32, 64), 0)
        run = _run(dev, inp, [64, 64, 128], False, False, seed=71)
        assert run["node"].xyz1, "the coordinates-only first layer did not take its moment path"
    else:
        inp = _inputs(dev, "E7", None, 12)
        run = _run(dev, inp, [32, 40, 24], False, False, xyz_first=False, seed=72)
        assert not run["node"].lin0
    _vs_f64(run, "E7/" + kind)
    _report()


# ---- E8: a duplicated cloud through the public layer ---------------------------------------------------------------------------------------------

def _node_of(out):
    fn = out.grad_fn
    for _ in range(4):
        if "MLPMax" in type(fn).__name__ or "MLPStack" in type(fn).__name__:
            return fn
        fn = fn.next_functions[0][0]
    raise AssertionError(type(out.grad_fn).__name__)


@pytest.mark.parametrize("compact", [True, None])
def test_duplicated_cloud_through_the_layer(dev, knobs, compact):
    """the second half of the points repeats the first (coordinates and features): FPS and the ball query tie exactly, a point and its twin are
    DISTINCT neighbours with identical rows.  Forward against the float64 oracle, gradients against the padded layer."""
    _geometry("default")
    N, K, radius = 128, 16, 0.4
    x = GC.e8_duplicated_cloud(N)
    half = np.random.default_rng(18).normal(size=(B, D, N // 2)).astype(np.float32)
    pts = np.concatenate([half, half], axis=2)
    st = np.zeros(B, np.int64)
    ws = seeded_weights([D + 3] + L3, 73)
    _, ref = R.PointNetSetAbstraction(S, radius, K, D + 3, L3, False, ws).forward(x, pts, st, f64=True)
    res = {}
    for mode in (False, compact):
        layer = PointNetSetAbstraction(S, radius, K, D + 3, L3, False).to(dev)
        layer.compact = mode
        with torch.no_grad():
            for conv, bn, (w, b_, g, bt) in zip(layer.mlp_convs, layer.mlp_bns, ws):
                conv.weight.copy_(torch.from_numpy(w).reshape(conv.weight.shape)); conv.bias.copy_(torch.from_numpy(b_))
                bn.weight.copy_(torch.from_numpy(g)); bn.bias.copy_(torch.from_numpy(bt))
        p = torch.from_numpy(pts).to(dev).requires_grad_(True)
        _, out = layer(torch.from_numpy(x).to(dev), p, torch.from_numpy(st).to(dev))
        assert (_node_of(out).compact is not None) == (mode is not False)
        if mode is None:
            assert layer._compact_on is True        # (measured: at most 0.75 of the slots are distinct neighbours)
        out.backward(torch.from_numpy(np.random.default_rng(19).normal(size=tuple(out.shape)).astype(np.float32)).to(dev))
        torch.cuda.synchronize()
        res[mode is not False] = (out.detach().cpu().numpy(), {n: q.grad.cpu().numpy() for n, q in layer.named_parameters()}, p.grad.cpu().numpy())
        WORST["f64 forward"] = max(WORST["f64 forward"], assert_close(res[mode is not False][0], ref, 1e-5, "E8 compact=%r forward vs f64 oracle" % (mode,)))
    (o0, g0, f0), (o1, g1, f1) = res[False], res[True]
    f = assert_close(o1, o0, 2e-6, "E8 compacted vs padded layer: forward")
    w = assert_close(f1, f0, 2e-5, "E8 compacted vs padded layer: dpoints")
    for n in g0:
        if "convs" in n and n.endswith("bias"):
            continue                                   # (conv bias under a train-mode BN: ~0 on both)
        w = max(w, assert_close(g1[n], g0[n], 2e-5, "E8 compacted vs padded layer: " + n))
    WORST["compacted vs padded forward"] = max(WORST["compacted vs padded forward"], f)
    WORST["compacted vs padded gradients"] = max(WORST["compacted vs padded gradients"], w)
    _report()
