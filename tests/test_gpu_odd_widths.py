"""The scalar kernel flavours -- the ones a width that is no multiple of 4, or a base pointer off a 16-byte boundary, selects -- held to float64.

Every row kernel has two flavours chosen on the host by one rule: float4 when the channel count is a multiple of 4 AND every base pointer is
16-byte aligned, element-wise otherwise (csrc/mlp_gemm.hip::check_dy / fill_asrc -> launch_gemm / launch_dw <.., VEC = false>; the
``v4 ? kernel<4> : kernel<1>`` launchers of csrc/bn_ops.hip).  The rest of the suite normalises multiples of 4 only; here every BatchNorm'd
width is odd or 2 mod 4, and aligned widths sit behind odd ones.

Bars (the project's own): against float64 -- tests/torch_ref.py::stack_routed on the kernel's own max / ReLU decisions -- forward 1e-5, every
gradient 2e-4 of max |ref| (the conv bias under a train-mode norm is "~0", as in test_gpu_geometry.py; under the frozen norm it is held
like the rest); the two orchestrations (stack.SharedMLPStack, mlp.SharedMLPMax) bit-identical to each other where no float atomics run;
bn_ops element-wise 1e-6, its reductions 2e-6; the oracle's float64 forward 1e-5.

A. Stacks (what each case is the smallest instance of, and why it fails if the flavour is wrong -- read from the kernels)
  O1  [13, 37, 21] on 37 groups of 24 rows: every operand loader of gemm_kernel / dw_kernel runs <VEC = false>: ld4s_or_zero masks the k-quad
      that straddles Kin (13 = 3 quads + 1, 37 = 9 + 1, 21 = 5 + 1) and finish_a4's ky / kz / kw zero the lanes past it.  A wrong mask adds
      the NEXT ROW's first elements (rows are Kin floats apart) into every product: the forward misses 1e-5 by orders of magnitude.  M = 888
      is 7 row tiles, the last of 120 rows; the statistics epilogue's column guard (n0 + c < Nout) on Nout = 37 and 21.  A_DY_MAX scalar:
      gout and argmax are read as [k .. k + 3] of a group's row of 21, guarded past Kin -- unguarded, the next group's winners route this one.
  O2  [22, 50, 30], no pool: rows 8- but not 16-byte aligned -- check_dy and fill_asrc must say "not vec" from C % 4 alone (every pointer IS
      aligned); a float4 load there is a misaligned-address fault or, clamped, the wrong columns.  bn_relu_kernel<1>, bn_bwd_reduce_kernel
      <1, false> with CG = 30: 8 row lanes and 16 idle threads.
  O3  grouped, D = 5 (cin 8), [30, 45], both column orders: the A_GROUP scalar loader (feats / xyz per element) in the forward and dW, the
      scatter dX onto feats under a scalar A_DY_DENSE operand; the order flag decides which 5 of the 8 weight columns meet the features.
  O4  [64, 50, 64] (and [16, 64, 50, 64]): aligned widths around an odd one.  Every buffer of a 64-wide layer is carved on a 256-byte
      boundary of its own (sa_mlp.hip::Carver; a tensor each in mlp.py), so those layers stay float4-legal and the flavours MIX: the dX of
      the 50 -> 64 layer runs the VEC A_DY_MAX loader (C = 64) into a ragged output of Nout = 50 columns with the 50-wide layer's
      BN-backward sums fused into its epilogue (EPI_STORE_RED: rows of 50 floats, the column guard at 50); its forward and dW are scalar by
      Kin = 50 although their dY side is float4-legal (launch_dw: vec = vdy && x.vec); the 64 -> 50 forward is float4 on the input side and
      ragged on the output side.  Only the 50-wide layer's own rows (cst[1..3], c12[1], dgamma / dbeta [2, 50]) sit 8 bytes off a 16-byte
      boundary, and they only ever reach scalar code.  A flavour chosen from ONE operand's width issues float4 loads on rows 200 bytes apart.
  O5  [16, 150] and [16, 301], dense and pooled K = 8: bn_bwd_reduce_kernel<1, *> with CG = 150, RL = 1 -- threads 150..255 have rl == RL
      and must contribute zeros to red[] -- and with two channel passes (256 + 45); red[(r * CG + g) * V + i] is read with r < RL only.
  O6  one layer of 7 channels straight on grouped input: A_DY_MAX scalar onto A_GROUP, Kin = 7 = one quad + 3.
  O7  group_all, [30, 45], N = 128 and 300: smallm.eligible / the library's plan must decline (widths no multiple of 8) -- the node is the row
      stack; bn_relu_max_kernel<1> on K = 128 and K >= 256 (bn_relu_max_split_kernel is v4-only).
  O1 and O3 again under the frozen norm (spec.eval_bn, running statistics away from (0, 1)); O1 and O4 with in-place gradient targets
  pre-filled with ones: the accumulate flavour of the folds and of bn_bwd_finalize_kernel on ragged C.
B. PointNetSetAbstraction [30, 45], PointNetSetAbstractionMsg [[10, 14], [18, 22]] and PointNetFeaturePropagation [50, 30] as a user builds
   them, forward against oracle.reference_np in float64; the first norm's running statistics against the oracle's layer statistics
   (bn_finalize_kernel on ragged C: one wave per channel, rows of 2 C floats).
C. bn_ops.hip through _lib, C in {1, 7, 50, 150, 301}: bn_relu_kernel<1>, bn_relu_max_kernel<1> (exact-arithmetic inputs with engineered
   ties: first index; a NaN wins and stays), bn_bwd_reduce_kernel<1, false / true> in all its operand forms with 1, 3 and more workgroups
   than row units (NaN-prefilled partials: an empty workgroup must write zeros) + bn_bwd_finalize_kernel with flag bits 0, 1, 2; psel ==
   scale * p.  Then C in {8, 64, 1028} aligned against the same values one float behind a 16-byte boundary: <4> against <1>.  Every
   tensor sits between NaN guards that must keep their bits.
D. What cannot take an odd width says so: papc_mlp_bwd_dx_max_f32 and the compacted dW return PAPC_E_UNSUPPORTED before any launch; the
   *_ok() predicates of the specialised paths say 0.

Measured on the MI355X, worst over the file (bar in brackets).  The scalar flavours meet every bar; no kernel, launcher or layout needed a fix.
  A  against float64: forward 3.09e-7 [1e-5] (O4), gradients 1.11e-6 [2e-4] (O3, coordinates first); frozen norm: 2.07e-7 / 3.77e-7;
     0 of up to 154 112 decisions per case differ from float64's own; the two orchestrations bit-identical (dfeats of O3 / O6 within 1e-5:
     float atomics); in-place targets: bit-equal to the autograd path + 1
  B  forward 3.63e-7 [1e-5] (FP, reference neighbours)
  C  element-wise 5.11e-8 [1e-6]; reductions and finalize 2.37e-7 [2e-6] (C = 301); <4> against <1>: element-wise outputs, argmax and psel
     identical, reductions 2.25e-7 [2e-6] (C = 1028: 0 -- one row lane in both flavours, the same order)
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import reference_np as R
from papc_amd import _lib, mlp, smallm
from papc_amd import functional as F
from papc_amd.layers import PointNetFeaturePropagation, PointNetSetAbstraction, PointNetSetAbstractionMsg
from papc_amd.mlp import StackSpec, shared_mlp_max
from papc_amd.synthetic import make_clouds, make_start_idx
from tests import torch_ref
from tests.util import assert_close, kernel_decisions, seeded_weights

pytestmark = pytest.mark.gpu

REL = 1e-5            # tests/test_gpu_mlp.py: forwards against float64
GTOL = 2e-4           # tests/test_gpu_mlp.py: gradients against float64
ELEM = 1e-6           # an fma and a compare per element (bn_relu, bn_relu_max): half an ulp of fp32 is 6e-8 of the value
RED = 2e-6            # tests/test_gpu_fp.py::test_three_interpolate_constant_neighbours_backward_is_a_reduction: fp32 sums of a few dozen terms
ATOMIC = 1e-5         # tests/test_gpu_cabi.py: the scatter dX adds with float atomics -- same terms, run-dependent order
EPS = 1e-5
NAMES = ["w", "b", "gamma", "beta"]
E_UNSUPPORTED = -2    # include/papc_hip.h: PAPC_E_UNSUPPORTED


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().double().cpu().numpy()


# ---- A. stacks against float64, both orchestrations -----------------------------------------------------------------------------------
# rows: plain input rows [G * K, chans[0]]; grouped: ball-query neighbourhoods of S centroids; group_all: identity rows, one group per cloud
CASES = {
    "O1": dict(form="rows", G=37, K=24, chans=[13, 37, 21], pool=True),
    "O2": dict(form="rows", G=300, K=1, chans=[22, 50, 30], pool=False),
    "O3-xyz_first": dict(form="grouped", B=2, N=256, S=32, K=16, D=5, mlp=[30, 45], xyz_first=True),
    "O3-feats_first": dict(form="grouped", B=2, N=256, S=32, K=16, D=5, mlp=[30, 45], xyz_first=False),
    "O4": dict(form="rows", G=16, K=16, chans=[64, 50, 64], pool=True),
    "O4-three_layers": dict(form="rows", G=16, K=16, chans=[16, 64, 50, 64], pool=True),
    "O5-150": dict(form="rows", G=512, K=1, chans=[16, 150], pool=False),
    "O5-301": dict(form="rows", G=512, K=1, chans=[16, 301], pool=False),
    "O5-150-pooled": dict(form="rows", G=64, K=8, chans=[16, 150], pool=True),
    "O5-301-pooled": dict(form="rows", G=64, K=8, chans=[16, 301], pool=True),
    "O6": dict(form="grouped", B=1, N=200, S=10, K=8, D=6, mlp=[7], xyz_first=True),
    "O7-128": dict(form="group_all", B=2, N=128, D=5, mlp=[30, 45], xyz_first=True),
    "O7-300": dict(form="group_all", B=2, N=300, D=5, mlp=[30, 45], xyz_first=True),
}
_HOST, _GROUPING = {}, {}


def _case(name):
    """the host arrays of one case, made once: everything the kernels and the float64 reference read"""
    if name in _HOST:
        return _HOST[name]
    c = dict(CASES[name])
    seed = 60 + sorted(CASES).index(name)
    rng = np.random.default_rng(200 + seed)
    c["x"] = c["xyz"] = c["feats"] = None
    if c["form"] == "rows":
        M, cin, widths = c["G"] * c["K"], c["chans"][0], c["chans"][1:]
        c["x"] = rng.normal(size=(M, cin)).astype(np.float32)
        c.update(B=1, N=M, S=c["G"], D=0, xyz_first=True)
    else:
        if c["form"] == "group_all":
            c.update(S=1, K=c["N"], pool=True)
        c.setdefault("pool", True)
        c["xyz"] = np.ascontiguousarray(make_clouds(c["B"], c["N"], 31 + c["N"]).transpose(0, 2, 1))
        c["feats"] = rng.normal(size=(c["B"], c["N"], c["D"])).astype(np.float32)
        cin, widths = c["D"] + 3, c["mlp"]
    c["M"], c["cin"], c["widths"] = c["B"] * c["S"] * c["K"], cin, list(widths)
    c["ws"] = seeded_weights([cin] + c["widths"], seed)
    # running statistics away from (0, 1), as tests/test_gpu_eval_backward.py seeds them: mean 0.1 N(0, 1), var U(0.5, 2)
    c["running"] = [((rng.normal(size=w) * 0.1).astype(np.float32), rng.uniform(0.5, 2.0, size=w).astype(np.float32)) for w in c["widths"]]
    c["gout"] = rng.normal(size=(c["B"] * c["S"] if c["pool"] else c["M"], c["widths"][-1])).astype(np.float32)
    _HOST[name] = c
    return c


def _grouping(dev, name, c):
    """(xyz, new_xyz, idx) on the device, made once per case: FPS + ball query as tests/test_gpu_geometry.py::_grouping"""
    if name not in _GROUPING:
        xyz = _t(c["xyz"], dev)
        if c["form"] == "group_all":
            _GROUPING[name] = (xyz, torch.zeros(c["B"], 1, 3, device=dev), None)
        else:
            _, new_xyz = F._fps_raw(xyz, c["S"], _t(make_start_idx(c["B"], c["N"], 1), dev))
            _GROUPING[name] = (xyz, new_xyz, F._ball_query_raw([0.3], [c["K"]], xyz, new_xyz)[0])
    return _GROUPING[name]


def _run(dev, monkeypatch, name, py_orch, eval_bn=False, inplace=False):
    """one forward + backward of the HIP stack under one orchestration -> everything a comparison needs"""
    monkeypatch.setattr(mlp, "_PY_ORCH", py_orch)
    c = _case(name)
    if inplace:
        params = [torch.nn.Parameter(_t(a, dev)) for tup in c["ws"] for a in tup]
        for p in params:
            p._papc_inplace_grad = True
            p.grad = torch.ones_like(p)
    else:
        params = [_t(a, dev).requires_grad_(True) for tup in c["ws"] for a in tup]
    bufs = [(_t(rm, dev), _t(rv, dev)) for rm, rv in c["running"]] if eval_bn else None
    before = [(a.clone(), b.clone()) for a, b in bufs] if eval_bn else None
    x = feats = idx = None
    if c["form"] == "rows":
        x = _t(c["x"], dev).requires_grad_(True)
        xyz = new_xyz = torch.zeros(1, 1, 3, device=dev)
    else:
        xyz, new_xyz, idx = _grouping(dev, name, c)
        feats = _t(c["feats"], dev).requires_grad_(True)
    spec = StackSpec(c["B"], c["N"], c["S"], c["K"], c["D"], c["xyz_first"], pool=c["pool"])
    spec.eval_bn = eval_bn
    assert not smallm.eligible(spec, xyz, feats, idx, x, params), "the planes path wants channel counts in multiples of 8"
    out = shared_mlp_max(spec, bufs, xyz, new_xyz, feats, idx, params, x_rows=x)
    fn = out.grad_fn
    node = type(fn).__name__
    assert node == ("SharedMLPMaxBackward" if py_orch else "SharedMLPStackBackward"), node      # the row stack, never PlanesMLPMax
    if not py_orch:
        assert not (fn.planes or fn.lin0 or fn.xyz1 or fn.nostore) and fn.compact is None, "a specialised plan took an odd width"
    assert (spec.grad_targets is not None) == inplace
    dec = kernel_decisions(out)
    out.backward(_t(c["gout"], dev))
    torch.cuda.synchronize()
    if eval_bn:
        for (a, b), (a0, b0) in zip(bufs, before):
            assert torch.equal(a, a0) and torch.equal(b, b0), "eval mode moved the running statistics"
    return {"out": out.detach(), "grads": [p.grad for p in params], "dfeats": None if feats is None else feats.grad,
            "dx": None if x is None else x.grad, "dec": dec, "idx": idx}


def _reference(dev, name, run, eval_bn):
    """the float64 chain on the kernel's own max / ReLU decisions (tests/torch_ref.py::stack_routed) and its autograd gradients"""
    c = _case(name)
    p64 = [[_t(a, dev).double().requires_grad_(True) for a in tup] for tup in c["ws"]]
    leaf = None
    if c["form"] == "rows":
        leaf = rows = _t(c["x"], dev).double().requires_grad_(True)
    else:
        xyz, new_xyz, idx = _grouping(dev, name, c)
        if idx is None:
            idx = torch.arange(c["N"], device=dev).view(1, 1, c["N"]).expand(c["B"], 1, c["N"])
        leaf = _t(c["feats"], dev).double().requires_grad_(True)
        rows = torch_ref.group(xyz.double(), new_xyz.double(), leaf, idx, c["xyz_first"]).reshape(c["M"], c["cin"])
    argmax, alive, masks = run["dec"]
    Kp = c["K"] if c["pool"] else 1
    if not c["pool"]:
        argmax = torch.zeros(c["M"], c["widths"][-1], dtype=torch.long, device=dev)
    running = [(_t(rm, dev).double(), _t(rv, dev).double()) for rm, rv in c["running"]] if eval_bn else None
    ref, stats = torch_ref.stack_routed(rows, [tuple(q) for q in p64], Kp, EPS, argmax, alive, masks, running=running)
    ref.backward(_t(c["gout"], dev).double())
    return ref, p64, leaf, stats


def _check_f64(dev, name, run, tag, eval_bn=False):
    """forward 1e-5, every gradient 2e-4 of max |ref|; -> (forward error, worst gradient error)"""
    c = _case(name)
    ref, p64, leaf, stats = _reference(dev, name, run, eval_bn)
    print("[odd] %s: decisions that differ from float64's own: %s" % (tag, stats))
    fwd = assert_close(_np(run["out"]), _np(ref), REL, tag + ": forward vs f64")
    worst = 0.0
    for l in range(len(c["widths"])):
        for j in range(4):
            got, want = _np(run["grads"][4 * l + j]), _np(p64[l][j].grad)
            if j == 1 and not eval_bn:
                # conv bias feeds a train-mode BN: its true gradient is exactly zero; both sides hold rounding noise (test_gpu_geometry.py)
                scale = float(np.abs(_np(p64[l][0].grad)).max())
                assert float(np.abs(got).max()) <= 1e-4 * scale, "%s db layer %d not ~0" % (tag, l)
                continue
            worst = max(worst, assert_close(got, want, GTOL, "%s: d%s layer %d vs f64" % (tag, NAMES[j], l)))
    gin = run["dx"] if run["dx"] is not None else run["dfeats"]
    worst = max(worst, assert_close(_np(gin), _np(leaf.grad), GTOL, tag + ": input gradient vs f64"))
    print("[odd] %s: forward %.2e (bar %.0e), gradients %.2e (bar %.0e) against float64" % (tag, fwd, REL, worst, GTOL))
    return fwd, worst


def _check_same(lib_, py, tag):
    """the two orchestrations issue the same launches: bit-identical where no float atomics run (tests/test_gpu_cabi.py)"""
    assert torch.equal(lib_["out"], py["out"]), tag + ": forward differs between the orchestrations"
    for i, (a, b) in enumerate(zip(lib_["grads"], py["grads"])):
        assert torch.equal(a, b), "%s: d%s layer %d differs between the orchestrations" % (tag, NAMES[i % 4], i // 4)
    if lib_["dx"] is not None:
        assert torch.equal(lib_["dx"], py["dx"]), tag + ": input gradient differs between the orchestrations"
    elif lib_["idx"] is None:       # identity rows: the scatter epilogue adds each dX entry once onto a zeroed buffer -- nothing to reorder
        assert torch.equal(lib_["dfeats"], py["dfeats"]), tag + ": dfeats differs between the orchestrations"
    else:
        assert float((lib_["dfeats"] - py["dfeats"]).abs().max()) <= ATOMIC * float(lib_["dfeats"].abs().max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_stack_vs_f64_both_orchestrations(dev, monkeypatch, name):
    res = {po: _run(dev, monkeypatch, name, po) for po in (False, True)}
    for po, r in res.items():
        _check_f64(dev, name, r, "%s %s" % (name, "python" if po else "library"))
    _check_same(res[False], res[True], name)


@pytest.mark.parametrize("name", ["O1", "O3-xyz_first", "O3-feats_first"])
def test_stack_eval_bn_vs_f64_both_orchestrations(dev, monkeypatch, name):
    """the frozen norm (spec.eval_bn, running statistics away from (0, 1)): no batch-mean terms, a conv bias gradient that is a real number"""
    res = {po: _run(dev, monkeypatch, name, po, eval_bn=True) for po in (False, True)}
    for po, r in res.items():
        _check_f64(dev, name, r, "%s eval %s" % (name, "python" if po else "library"), eval_bn=True)
    _check_same(res[False], res[True], name + " eval")


@pytest.mark.parametrize("name", ["O1", "O4", "O4-three_layers"])
def test_stack_inplace_targets_add_onto_ones(dev, monkeypatch, name):
    """every parameter opted in to in-place accumulation with .grad = 1: the backward adds with ONE fp32 add per element (fold.h `*o + s`,
    bn_bwd_finalize_kernel `dbeta[c] + (float) s1`), the same s the autograd path returns -- the bit equality tests/test_gpu_inplace.py holds
    a stack without a gather-add or planes layer to.  (With all four targets of a layer given, db is folded in place too: nodeparts.LayerSlots.)"""
    base = _run(dev, monkeypatch, name, False)
    got = _run(dev, monkeypatch, name, False, inplace=True)
    assert torch.equal(base["out"], got["out"]) and torch.equal(base["dx"], got["dx"])
    for i, (g, gi) in enumerate(zip(base["grads"], got["grads"])):
        what = "%s: in-place d%s layer %d" % (name, NAMES[i % 4], i // 4)
        if i % 4 == 1:      # (the bias under a train-mode norm: rounding noise around an exact zero, folded and added like any other db)
            assert float(g.abs().max()) <= 1e-4 * float(base["grads"][i - 1].abs().max())
        assert torch.equal(gi, g + 1), "%s differs from the autograd path + 1 by %.3e" % (what, float((gi - (g + 1)).abs().max()))


# ---- B. the layer classes with user-chosen odd widths, forward against the oracle ----------------------------------------------------------

def _load(convs, bns, ws):
    with torch.no_grad():
        for conv, bn, (w, b, g, bt) in zip(convs, bns, ws):
            conv.weight.copy_(torch.from_numpy(w).reshape(conv.weight.shape))
            conv.bias.copy_(torch.from_numpy(b))
            bn.weight.copy_(torch.from_numpy(g))
            bn.bias.copy_(torch.from_numpy(bt))


def _check_running(bn, y64, what):
    """paddle's momentum rule (momentum 0.9 weighs the OLD value; fresh buffers are 0 / 1) on the float64 batch statistics of the layer's
    pre-BN output ``y64`` [M, C]: biased variance"""
    assert_close(_np(bn.running_mean), 0.1 * y64.mean(0), REL, what + ": running mean")
    assert_close(_np(bn.running_var), 0.9 + 0.1 * y64.var(0), REL, what + ": running var (biased)")


def test_sa_layer_odd_widths_vs_oracle(dev):
    B, N, S, K, D, widths = 3, 300, 20, 16, 5, [30, 45]
    x, st = make_clouds(B, N, 77 + N), make_start_idx(B, N, 3)
    pts = np.random.default_rng(9).normal(size=(B, D, N)).astype(np.float32)
    ws = seeded_weights([D + 3] + widths, 5)
    ref_xyz, ref, acts = R.PointNetSetAbstraction(S, 0.3, K, D + 3, widths, False, ws).forward(x, pts, st, f64=True, return_all=True)
    layer = PointNetSetAbstraction(S, 0.3, K, D + 3, widths, False).to(dev)
    _load(layer.mlp_convs, layer.mlp_bns, ws)
    got_xyz, got = layer(_t(x, dev), _t(pts, dev), _t(st, dev))
    assert tuple(got.shape) == (B, widths[-1], S) and np.array_equal(got_xyz.cpu().numpy(), ref_xyz)
    err = assert_close(_np(got), ref, REL, "SA [30, 45] vs f64 oracle")
    _check_running(layer.mlp_bns[0], np.asarray(acts[0][0], np.float64), "SA [30, 45]")
    print("[odd] SA layer forward %.2e against the float64 oracle" % err)


def test_sa_msg_layer_odd_widths_vs_oracle(dev):
    B, N, S, radii, ks, mlps = 2, 256, 32, [0.2, 0.4], [8, 16], [[10, 14], [18, 22]]
    x, st = make_clouds(B, N, 15), make_start_idx(B, N, 4)
    pts = np.random.default_rng(2).normal(size=(B, 3, N)).astype(np.float32)
    ws = [seeded_weights([6] + m, 20 + i) for i, m in enumerate(mlps)]
    ref_xyz, ref = R.PointNetSetAbstractionMsg(S, radii, ks, 3, mlps, ws).forward(x, pts, st, f64=True)
    layer = PointNetSetAbstractionMsg(S, radii, ks, 3, mlps).to(dev)
    for i in range(len(mlps)):
        _load(layer.conv_blocks[i], layer.bn_blocks[i], ws[i])
    got_xyz, got = layer(_t(x, dev), _t(pts, dev), _t(st, dev))
    assert tuple(got.shape) == (B, 14 + 22, S) and np.array_equal(got_xyz.cpu().numpy(), ref_xyz)
    err = assert_close(_np(got), ref, REL, "MSG [[10, 14], [18, 22]] vs f64 oracle")
    # the first norm of each branch: the oracle's grouped rows [feats, xyz] (reference_np.PointNetSetAbstractionMsg.forward) through its conv
    xyz, points = np.ascontiguousarray(np.transpose(x, (0, 2, 1))), np.ascontiguousarray(np.transpose(pts, (0, 2, 1)))
    new_xyz = R.index_points(xyz, R.farthest_point_sample(xyz, S, st, 1.0))
    for i, (radius, K) in enumerate(zip(radii, ks)):
        gi = R.query_ball_point(radius, K, xyz, new_xyz)
        rows = np.concatenate([R.index_points(points, gi), R.index_points(xyz, gi) - new_xyz.reshape(B, S, 1, 3)], axis=-1).reshape(B * S * K, 6)
        _check_running(layer.bn_blocks[i][0], R.conv1x1_rows(rows, ws[i][0][0], ws[i][0][1], f64=True), "MSG branch %d" % i)
    print("[odd] MSG layer forward %.2e against the float64 oracle" % err)


@pytest.mark.parametrize("neighbours", ["reference", "nearest"])
def test_fp_layer_odd_widths_vs_oracle(dev, neighbours):
    B, N, S, D1, D2, widths = 2, 128, 16, 6, 21, [50, 30]
    rng = np.random.default_rng(7)
    x1 = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    x2 = np.ascontiguousarray(x1[:, rng.permutation(N)[:S]])
    p1, p2 = rng.normal(size=(B, D1, N)).astype(np.float32), rng.normal(size=(B, D2, S)).astype(np.float32)
    ws = seeded_weights([D1 + D2] + widths, 5)
    xyz1, xyz2 = np.ascontiguousarray(x1.transpose(0, 2, 1)), np.ascontiguousarray(x2.transpose(0, 2, 1))
    ref, interp_ref = R.PointNetFeaturePropagation(D1 + D2, widths, ws, neighbours).forward(xyz1, xyz2, p1, p2, f64=True, return_interp=True)
    fp = PointNetFeaturePropagation(D1 + D2, widths, neighbours=neighbours).to(dev)
    _load(fp.mlp_convs, fp.mlp_bns, ws)
    interp = fp.interpolate(_t(xyz1, dev).transpose(1, 2), _t(xyz2, dev).transpose(1, 2), _t(p2, dev).transpose(1, 2))
    assert np.array_equal(interp.cpu().numpy(), interp_ref)          # the interpolation itself is bit-exact (21 channels: scalar lanes)
    got = fp(_t(xyz1, dev), _t(xyz2, dev), _t(p1, dev), _t(p2, dev))
    assert tuple(got.shape) == (B, widths[-1], N)
    err = assert_close(_np(got), ref, REL, "FP [50, 30] vs f64 oracle")
    rows = np.concatenate([np.transpose(p1, (0, 2, 1)), interp_ref], axis=-1).reshape(B * N, D1 + D2)
    _check_running(fp.mlp_bns[0], R.conv1x1_rows(rows, ws[0][0], ws[0][1], f64=True), "FP [50, 30]")
    print("[odd] FP layer (%s) forward %.2e against the float64 oracle" % (neighbours, err))


# ---- C. the bn_ops.hip entry points directly ---------------------------------------------------------------------------------------------

PAD = 8       # floats of guard on either side of a placed tensor


class Placed:
    """``a`` copied ``off`` floats behind a 16-byte boundary of a larger device buffer (off = 0: aligned, the launchers' <4> flavours where
    C % 4 == 0; off = 1: their aligned16() test picks <1>), with PAD + off guard elements in front and PAD behind that must keep their bits"""

    def __init__(self, dev, a, off, fill=None):
        a = np.ascontiguousarray(a)
        self.n, self.lo = a.size, PAD + off
        self.guard = float("nan") if a.dtype == np.float32 else -7
        self.buf = torch.full((self.lo + self.n + PAD,), self.guard, dtype=torch.from_numpy(a).dtype, device=dev)
        self.t = self.buf[self.lo: self.lo + self.n].view(a.shape)
        self.t.copy_(torch.from_numpy(a) if fill is None else torch.full_like(self.t, fill))
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == (4 * off) % 16 and PAD % 4 == 0

    def ptr(self):
        return self.t.data_ptr()

    def check_guards(self, what):
        g = torch.cat([self.buf[:self.lo], self.buf[self.lo + self.n:]])
        assert bool(torch.isnan(g).all() if g.is_floating_point() else (g == self.guard).all()), what + ": a store outside the tensor"


def _out(dev, shape, off, dtype=np.float32):
    """an output tensor pre-filled with NaN (int32: -7): whatever the kernel leaves unwritten shows"""
    return Placed(dev, np.empty(shape, dtype), off, fill=float("nan") if dtype == np.float32 else -7)


def _bn_consts(rng, C):
    """(mean, invstd, scale, shift) float32 [C]: a quarter of the scales negative, as seeded_weights' gammas"""
    mean = (rng.normal(size=C) * 0.3).astype(np.float32)
    invstd = rng.uniform(0.5, 2.0, size=C).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, size=C) * rng.choice([1.0, 1.0, 1.0, -1.0], size=C)
    scale = (gamma * invstd).astype(np.float32)
    shift = (rng.normal(size=C) * 0.2).astype(np.float32)
    return mean, invstd, scale, shift


def _relu_max(dev, y, scale, shift, G, K, C, off):
    """papc_bn_relu_max_f32 -> (out [G, C], argmax [G, C]) on the host"""
    ty, ts, th = Placed(dev, y, off), Placed(dev, scale, off), Placed(dev, shift, off)
    o, am = _out(dev, (G, C), off), _out(dev, (G, C), off, np.int32)
    _lib.check(_lib.load().papc_bn_relu_max_f32(ty.ptr(), ts.ptr(), th.ptr(), G, K, C, o.ptr(), am.ptr(), _lib.stream_ptr()), "papc_bn_relu_max_f32")
    torch.cuda.synchronize()
    o.check_guards("bn_relu_max out")
    am.check_guards("bn_relu_max argmax")
    return o.t.cpu().numpy(), am.t.cpu().numpy()


def _relu(dev, y, scale, shift, M, C, off):
    ty, ts, th = Placed(dev, y, off), Placed(dev, scale, off), Placed(dev, shift, off)
    o = _out(dev, (M, C), off)
    _lib.check(_lib.load().papc_bn_relu_f32(ty.ptr(), ts.ptr(), th.ptr(), M, C, o.ptr(), _lib.stream_ptr()), "papc_bn_relu_f32")
    torch.cuda.synchronize()
    o.check_guards("bn_relu out")
    return o.t.cpu().numpy()


def _z64(y, scale, shift):
    return np.maximum(scale.astype(np.float64) * y.astype(np.float64) + shift.astype(np.float64), 0.0)


def _lattice(rng, G, K, C):
    """inputs on which scale * y + shift is EXACT in fp32 (quarters times halves plus quarters, all small): the maximum ties among many rows
    and float64 says without ambiguity which index is first.  Row 1 of every group (K >= 3) is the extreme of every channel -- y = 5
    sign(scale) against |y| <= 4 elsewhere -- and the last row is its copy: the winner is index 1, never K - 1.  One channel has scale == 0:
    all K rows tie at relu(shift), index 0 wins."""
    y = (rng.integers(-16, 17, size=(G, K, C)) / 4.0).astype(np.float32)
    scale = rng.choice([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5], size=C).astype(np.float32)
    shift = (rng.integers(-4, 5, size=C) / 4.0).astype(np.float32)
    dead = C // 2
    if K >= 3:
        y[:, 1, :] = 5.0 * np.sign(scale)
        y[:, K - 1, :] = y[:, 1, :]
    if C > 1:
        scale[dead] = 0.0
    return y.reshape(G * K, C), scale, shift, dead


@pytest.mark.parametrize("C", [1, 7, 50, 150, 301])
def test_bn_relu_and_bn_relu_max_scalar_flavour(dev, C):
    """bn_relu_kernel<1> and bn_relu_max_kernel<1> (C % 4 != 0; K = 300 too: the split kernel is v4-only): values within 1e-6 of float64, the
    first index attaining the maximum on exact ties, a NaN wins and stays"""
    G = 5
    worst = 0.0
    for K in (1, 7, 300):
        rng = np.random.default_rng(1000 * C + K)
        # (a) exact inputs: values and indices equal float64's, element for element
        y, scale, shift, dead = _lattice(rng, G, K, C)
        z = _z64(y, scale, shift)
        out, am = _relu_max(dev, y, scale, shift, G, K, C, 0)
        zg = z.reshape(G, K, C)
        assert np.array_equal(out.astype(np.float64), zg.max(1)), (C, K, "lattice values")
        assert np.array_equal(am, zg.argmax(1)), (C, K, "argmax is not the first index attaining the maximum")
        if K >= 3:
            live = scale != 0
            assert (am[:, live] == 1).all() and (am[:, ~live] == 0).all()
        assert np.array_equal(_relu(dev, y, scale, shift, G * K, C, 0).astype(np.float64), z), (C, K, "bn_relu lattice values")
        # (b) random inputs with two identical rows per group: within 1e-6 of float64, the copy never wins
        y = rng.normal(size=(G, K, C)).astype(np.float32)
        _, _, scale, shift = _bn_consts(rng, C)
        if C > 1:
            scale[dead] = 0.0
        j1, j2 = (K // 3, K - 1) if K >= 2 else (0, 0)
        y[:, j2, :] = y[:, j1, :]
        y = y.reshape(G * K, C)
        z = _z64(y, scale, shift)
        zg = z.reshape(G, K, C)
        ref = zg.max(1)
        out, am = _relu_max(dev, y, scale, shift, G, K, C, 0)
        tol = ELEM * float(np.abs(ref).max())
        worst = max(worst, _rel(out, ref))
        assert float(np.abs(out - ref).max()) <= tol, (C, K, "bn_relu_max values")
        assert am.min() >= 0 and am.max() < K
        at = np.take_along_axis(zg, am[:, None, :].astype(np.int64), 1)[:, 0]
        assert float(np.abs(at - ref).max()) <= tol, (C, K, "argmax does not point at the maximum")
        if K >= 2:
            assert (am != j2).all(), (C, K, "the later of two identical rows won")
        if C > 1:
            assert (am[:, dead] == 0).all(), (C, K, "scale == 0: every row ties, index 0 is first")
        got = _relu(dev, y, scale, shift, G * K, C, 0)
        worst = max(worst, _rel(got, z))
        assert float(np.abs(got - z).max()) <= ELEM * float(np.abs(z).max()), (C, K, "bn_relu values")
        # (c) one NaN: it wins its (group, channel) and stays to the last row; nothing else moves
        kn, cn = K // 2, C - 1
        yn = y.copy()
        yn[2 * K + kn, cn] = np.nan
        out_n, am_n = _relu_max(dev, yn, scale, shift, G, K, C, 0)
        assert np.isnan(out_n[2, cn]) and am_n[2, cn] == kn, (C, K, "a NaN must win and stay")
        keep = np.ones((G, C), bool)
        keep[2, cn] = False
        assert np.array_equal(out_n[keep], out[keep]) and np.array_equal(am_n[keep], am[keep])
    print("[odd] bn_relu / bn_relu_max <1> C=%d: %.2e of max |ref| against float64 (bar %.0e)" % (C, worst, ELEM))


def _reduce_inputs(rng, M, K, C):
    """y [M, C], dense dz [M, C], gout / argmax [M / K, C], the BN constants; ysel = y at the argmax"""
    G = M // K
    mean, invstd, scale, shift = _bn_consts(rng, C)
    y = (rng.normal(size=(M, C)) + mean).astype(np.float32)
    d = {"y": y, "dz": rng.normal(size=(M, C)).astype(np.float32), "gout": rng.normal(size=(G, C)).astype(np.float32),
         "argmax": rng.integers(0, K, size=(G, C)).astype(np.int32), "mean": mean, "invstd": invstd, "scale": scale, "shift": shift}
    rows = (np.arange(G)[:, None] * K + d["argmax"]).astype(np.int64)
    d["ysel"] = np.take_along_axis(y, rows, 0)
    return d


def _reduce_ref(d, dense):
    """float64 (sum p, sum p xhat) per channel and psel = scale * p as ONE fp32 product"""
    yv, g = (d["y"], d["dz"]) if dense else (d["ysel"], d["gout"])
    f8 = lambda a: a.astype(np.float64)     # noqa: E731
    z = f8(d["scale"]) * f8(yv) + f8(d["shift"])        # (an exact product and one rounding: the sign is the sign of the kernel's fmaf)
    p = np.where(z > 0, g, np.float32(0.0)).astype(np.float32)
    s1 = f8(p).sum(0)
    s2 = (f8(p) * (f8(yv) - f8(d["mean"])) * f8(d["invstd"])).sum(0)
    return s1, s2, d["scale"][None, :] * p


MODES = ("dense", "max_gather", "max_ysel", "reduce_max", "reduce_max_psel")


def _reduce(dev, d, mode, M, K, C, n_parts, off):
    """one reduce launch -> (partials [n_parts, 2, C] on the host, psel or None, the device partials for the finalize)"""
    lib, st = _lib.load(), _lib.stream_ptr()
    P = {k: Placed(dev, d[k], off) for k in ("y", "dz", "gout", "argmax", "ysel", "mean", "invstd", "scale", "shift")}
    red = _out(dev, (n_parts, 2, C), off)
    psel = None
    cst = (P["mean"].ptr(), P["invstd"].ptr(), P["scale"].ptr(), P["shift"].ptr())
    if mode == "dense":
        rc = lib.papc_bn_bwd_reduce_f32(0, P["dz"].ptr(), None, None, 1, P["y"].ptr(), *cst, M, C, n_parts, red.ptr(), st)
    elif mode == "max_gather":      # dz == NULL: y gathered at the argmax, element by element
        rc = lib.papc_bn_bwd_reduce_f32(1, None, P["gout"].ptr(), P["argmax"].ptr(), K, P["y"].ptr(), *cst, M, C, n_parts, red.ptr(), st)
    elif mode == "max_ysel":        # dz = ysel: y is never read (NULL is legal then)
        rc = lib.papc_bn_bwd_reduce_f32(1, P["ysel"].ptr(), P["gout"].ptr(), P["argmax"].ptr(), K, None, *cst, M, C, n_parts, red.ptr(), st)
    else:
        if mode == "reduce_max_psel":
            psel = _out(dev, (M // K, C), off)
        rc = lib.papc_bn_bwd_reduce_max_f32(P["ysel"].ptr(), P["gout"].ptr(), K, *cst, M, C, n_parts, red.ptr(), None if psel is None else psel.ptr(), st)
    _lib.check(rc, "bn_bwd_reduce (%s)" % mode)
    torch.cuda.synchronize()
    red.check_guards("reduce partials (%s)" % mode)
    if psel is not None:
        psel.check_guards("psel")
    return red.t.cpu().numpy(), None if psel is None else psel.t.cpu().numpy(), red


def _finalize(dev, red, n_parts, M, C, flag, old):
    """papc_bn_bwd_finalize_f32 with accumulate bits ``flag`` onto dgamma = dbeta = ``old`` -> (dgamma, dbeta, c1, c2) on the host"""
    dg, db = Placed(dev, old[0], 0), Placed(dev, old[1], 0)
    c12 = _out(dev, (2, C), 0)
    _lib.check(_lib.load().papc_bn_bwd_finalize_f32(red.ptr(), n_parts, M, C, dg.ptr(), db.ptr(), c12.ptr(), c12.ptr() + 4 * C, flag, _lib.stream_ptr()),
               "papc_bn_bwd_finalize_f32")
    torch.cuda.synchronize()
    for p in (dg, db, c12):
        p.check_guards("finalize")
    c = c12.t.cpu().numpy()
    return dg.t.cpu().numpy(), db.t.cpu().numpy(), c[0], c[1]


def _rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


@pytest.mark.parametrize("C", [1, 7, 50, 150, 301])
def test_bn_bwd_reduce_scalar_flavour_and_finalize(dev, C):
    """bn_bwd_reduce_kernel<1, false / true> on 37 rows (dense) and 5 groups of 7 (MAX) with 1, 3 and more workgroups than row units, each
    followed by the finalize with accumulate bits 0, 1 and 2"""
    worst = 0.0
    for mode in MODES:
        dense = mode == "dense"
        M, K = (37, 1) if dense else (35, 7)
        units = M // K
        rng = np.random.default_rng(77 * C + MODES.index(mode))
        d = _reduce_inputs(rng, M, K, C)
        s1, s2, psel_ref = _reduce_ref(d, dense)
        for n_parts in (1, 3, units + 3):
            part, psel, red = _reduce(dev, d, mode, M, K, C, n_parts, 0)
            assert np.isfinite(part).all(), (C, mode, n_parts, "a partial row was left unwritten")
            per = (units + n_parts - 1) // n_parts
            empty = [b for b in range(n_parts) if b * per >= units]
            assert (n_parts <= units) == (not empty)
            assert all(not part[b].any() for b in empty), (C, mode, n_parts, "an empty workgroup must write zeros")
            tot = part.astype(np.float64).sum(0)
            worst = max(worst, _rel(tot[0], s1), _rel(tot[1], s2))
            assert _rel(tot[0], s1) <= RED and _rel(tot[1], s2) <= RED, (C, mode, n_parts, "partial sums")
            if psel is not None:
                assert np.array_equal(psel, psel_ref), (C, mode, n_parts, "psel != scale * p")
            old = rng.normal(size=(2, C)).astype(np.float32)
            for flag in (0, 1, 2):
                dg, db, c1, c2 = _finalize(dev, red, n_parts, M, C, flag, old)
                acc = 1.0 if flag & 1 else 0.0
                want = (s2 + acc * old[0], s1 + acc * old[1], s1 / M * (0.0 if flag & 2 else 1.0), s2 / M * (0.0 if flag & 2 else 1.0))
                for nm, got, ref in zip(("dgamma", "dbeta", "c1", "c2"), (dg, db, c1, c2), want):
                    if flag & 2 and nm in ("c1", "c2"):
                        assert not got.any(), (C, mode, nm, "the eval-mode norm has no batch-mean terms")
                        continue
                    scale_ref = ref if not acc else np.concatenate([ref, s1, s2])      # (an accumulated sum is read on the scale of its terms)
                    e = float(np.abs(got - ref).max()) / max(float(np.abs(scale_ref).max()), 1e-30)
                    worst = max(worst, e)
                    assert e <= RED, (C, mode, n_parts, flag, nm, e)
    print("[odd] bn_bwd_reduce <1> + finalize C=%d: %.2e of max |ref| against float64 (bar %.0e)" % (C, worst, RED))


@pytest.mark.parametrize("C", [8, 64, 1028])
def test_bn_ops_vector_flavour_equals_scalar_flavour(dev, C):
    """the same values once on 16-byte aligned tensors (the <4> flavours; C = 1028: their second channel pass) and once placed one float
    behind a 16-byte boundary (the launchers' aligned16() test picks <1>): element-wise outputs and argmax identical, reductions within 2e-6"""
    rng = np.random.default_rng(5 * C)
    G, worst = 5, 0.0
    for K in (7, 300):        # (K = 300, aligned: few long groups -- bn_relu_max_split_kernel)
        y = rng.normal(size=(G, K, C)).astype(np.float32)
        y[:, K - 1, :] = y[:, K // 3, :]
        y = y.reshape(G * K, C)
        _, _, scale, shift = _bn_consts(rng, C)
        scale[C // 2] = 0.0
        (o4, a4), (o1, a1) = (_relu_max(dev, y, scale, shift, G, K, C, off) for off in (0, 1))
        assert np.array_equal(o4, o1) and np.array_equal(a4, a1), (C, K, "bn_relu_max <4> vs <1>")
        assert np.array_equal(_relu(dev, y, scale, shift, G * K, C, 0), _relu(dev, y, scale, shift, G * K, C, 1)), (C, K, "bn_relu <4> vs <1>")
    for mode in MODES:
        dense = mode == "dense"
        M, K = (37, 1) if dense else (35, 7)
        d = _reduce_inputs(rng, M, K, C)
        s1, s2, psel_ref = _reduce_ref(d, dense)
        for n_parts in (1, 3):
            (p4, q4, _), (p1, q1, _) = (_reduce(dev, d, mode, M, K, C, n_parts, off) for off in (0, 1))
            t4, t1 = p4.astype(np.float64).sum(0), p1.astype(np.float64).sum(0)
            for j, s in enumerate((s1, s2)):
                worst = max(worst, _rel(t4[j], t1[j]))
                assert _rel(t4[j], t1[j]) <= RED, (C, mode, n_parts, "<4> vs <1>")
                assert _rel(t4[j], s) <= RED and _rel(t1[j], s) <= RED, (C, mode, n_parts, "against float64")
            if q4 is not None:
                assert np.array_equal(q4, q1) and np.array_equal(q4, psel_ref), (C, mode, "psel <4> vs <1>")
    print("[odd] bn_ops <4> vs <1> C=%d: reductions differ by %.2e (bar %.0e); element-wise outputs and argmax identical" % (C, worst, RED))


# ---- D. refusals --------------------------------------------------------------------------------------------------------------------------

ODD = (7, 21, 30, 37, 45, 50, 150, 301)      # the normalised widths of groups A and B that are no multiple of 4


def _last_error():
    return _lib.load().papc_last_error_string().decode("utf-8", "replace")


def test_sparse_max_dx_refuses_odd_widths(dev):
    """papc_mlp_bwd_dx_max_f32 has a float4 flavour only: Cout % 16 != 0 (or Cin % 4 != 0) is PAPC_E_UNSUPPORTED before anything is launched
    -- mlp.py routes round it (``cL % 16 == 0 and cLi % 4 == 0``), sa_mlp.hip plans it only where papc_mlp_max_nostore_ok says yes"""
    lib = _lib.load()
    M, K = 256, 16
    for cin, cout in ((30, 45), (32, 45), (30, 48), (50, 64)):
        z = lambda *s: torch.zeros(*s, device=dev)       # noqa: E731
        psel, am, x, sc, sh = z(M // K, cout), torch.zeros(M // K, cout, dtype=torch.int32, device=dev), z(M, cin), z(cin), z(cin)
        wcat, hb, dx = z(cin, cout + cin), z(cin), torch.full((M, cin), 3.0, device=dev)
        rc = lib.papc_mlp_bwd_dx_max_f32(psel.data_ptr(), am.data_ptr(), K, x.data_ptr(), cin, sc.data_ptr(), sh.data_ptr(), wcat.data_ptr(),
                                         hb.data_ptr(), M, cin, cout, dx.data_ptr(), None, _lib.stream_ptr())
        assert rc == E_UNSUPPORTED and "Cout" in _last_error(), (cin, cout, rc, _last_error())
        with pytest.raises(_lib.PapcError, match="Cout"):
            _lib.check(rc, "papc_mlp_bwd_dx_max_f32")
        torch.cuda.synchronize()
        assert bool((dx == 3.0).all()), "a refused call wrote its output"


def test_compacted_dw_refuses_a_width_other_than_128(dev):
    """papc_mlp_bwd_dw_f32 with a compacted dY source (papc_bwd_dy.wrow): dw_rowsx_kernel's compacted flavours or nothing -- a 50-channel
    input is PAPC_E_UNSUPPORTED, named in the message; compact.stack_ok / papc_mlp_compact_ok keep the stacks away from it"""
    lib = _lib.load()
    M, K = 256, 16
    for cin, cout in ((50, 128), (30, 45), (128, 50)):
        z = lambda *s: torch.zeros(*s, device=dev)       # noqa: E731
        dy = _lib.BwdDy()
        y, dz, cst, c12 = z(M, cout), z(M, cout), z(4, cout), z(2, cout)
        dy.dz_mode, dy.dz, dy.K = 0, dz.data_ptr(), 1
        dy.set_bn(y, cst, c12)
        wrow, seg, rows = z(M), torch.zeros(M, dtype=torch.int32, device=dev), torch.full((1,), M, dtype=torch.int32, device=dev)
        dy.wrow, dy.seg_grp, dy.rows_dev = wrow.data_ptr(), seg.data_ptr(), rows.data_ptr()
        x, sc, sh = z(M, cin), z(cin), z(cin)
        part = torch.full((1, cout * cin + cout), 3.0, device=dev)
        rc = lib.papc_mlp_bwd_dw_f32(ctypes.byref(dy), mlp.A_BNRELU, x.data_ptr(), cin, None, sc.data_ptr(), sh.data_ptr(), M, cin, cout, 256,
                                     part.data_ptr(), part.data_ptr() + 4 * cout * cin, part.shape[1], _lib.stream_ptr())
        assert rc == E_UNSUPPORTED and ("Cin=%d" % cin) in _last_error() and ("Cout=%d" % cout) in _last_error(), (cin, cout, rc, _last_error())
        torch.cuda.synchronize()
        assert bool((part == 3.0).all()), "a refused call wrote its output"


def test_specialised_paths_decline_odd_widths():
    """every *_ok() predicate says 0 for the odd widths of this file, at row counts large enough that the width alone decides"""
    lib = _lib.load()
    M = 1 << 17
    for w in ODD:
        for couts in ([w, 256], [128, w], [w, w]):
            assert lib.papc_mlp_compact_ok(M, 16, 2, (ctypes.c_int * 2)(*couts)) == 0, couts
        assert lib.papc_mlp_xyz_ok(M, w, 64) == 0 and lib.papc_mlp_xyz_ok(M, 64, w) == 0
        for K in (32, 64, 128):
            assert lib.papc_mlp_max_nostore_ok(M, w, 128, K) == 0 and lib.papc_mlp_max_nostore_ok(M, 64, w, K) == 0
        assert lib.papc_cloud_concat_k_ok(w, 64, 64) == 0 and lib.papc_cloud_concat_k_ok(64, w, 64) == 0 and lib.papc_cloud_concat_k_ok(64, 64, w) == 0
        for ok in (lib.papc_kdconv_ok, lib.papc_kdbn_ok):
            assert ok(64, w, 64) == 0 and ok(64, 32, w) == 0
    # (the stacks of group A themselves: their own row counts)
    assert lib.papc_mlp_compact_ok(1024, 16, 2, (ctypes.c_int * 2)(30, 45)) == 0
    assert lib.papc_mlp_max_nostore_ok(256, 50, 64, 16) == 0 and lib.papc_mlp_xyz_ok(888, 37, 21) == 0
