"""Shared pointwise MLP stack -- relu(bn(conv1x1(x))) x L, then max over the K rows of each group -- as ONE
autograd node driving the HIP kernels (include/papc_hip.h: papc_mlp_gemm_f32, papc_bn_finalize_f32,
papc_bn_relu_max_f32 and the papc_*bwd* family).

Reference: /root/reference/PAPC/models/layers/pointnet2_basic_layers.py:214-219 (SSG), :271-276 (MSG),
/root/reference/PAPC/models/classify/pointnet_base/pointnet_base.py:7-25,44 (PointNet-Basic Conv1D stack).

What is stored between forward and backward: only the pre-BN conv outputs y_l [M,C_l], the per-channel BN
constants and the argmax of the final max.  Grouped input rows, BN+ReLU activations and dY are recomputed
inside the operand loads of the MFMA kernels.
"""
import ctypes

import torch

from . import _lib
from ._lib import BwdDy, BwdRed, GroupMax, GroupSrc, ReduceJob, ScatterDst, check, cst_ptrs, ptr, stream_ptr
from .nodeparts import DwPartials, LayerSlots, bn_bwd_sums, identity_bn, launch_batched
from .nodeparts import grad_targets_of, _dw_rows_per_chunk      # noqa: F401  (re-exported: tests and tools import them from here)

A_PLAIN, A_BNRELU, A_GROUP, A_XYZ = 0, 1, 2, 6
DZ_DENSE, DZ_MAX = 0, 1


class StackSpec:
    """Static description of one stack invocation (not a tensor; passed through autograd untouched)."""

    def __init__(self, B, N, S, K, D, xyz_first, eps=1e-5, momentum=0.9, cut_gather_grad=False, pool=True, eval_bn=False):
        self.B, self.N, self.S, self.K, self.D = B, N, S, K, D
        # pool=False: no max over K -- the stack returns relu(bn_L(.)) for every row (PointNetFeaturePropagation's
        # Conv1D stack, pointnet2_basic_layers.py:330-333)
        self.pool = bool(pool)
        # eval_bn=True: the BatchNorms normalise with their RUNNING statistics and leave them untouched (a registered norm of the
        # source under model.eval(): pointnet_base.py:8-24, pillars.py:24); needs bn_buffers.  The SA / FP layers never set it: the
        # source keeps their norms in plain lists, so .eval() never reaches them (pointnet2_basic_layers.py:185-191).
        self.eval_bn = bool(eval_bn)
        self.xyz_first = bool(xyz_first)
        self.eps, self.momentum = float(eps), float(momentum)
        self.cut_gather_grad = cut_gather_grad
        self.M = B * S * K
        # optional: per-parameter gradient buffers (contiguous, same shape as the parameter) that the backward
        # accumulates into directly instead of returning gradients to autograd (see grad_targets_of)
        self.grad_targets = None
        # optional: W^T operands precomputed for THIS forward pass by the caller (precompute_wt); None = transpose in the backward
        self.wt_table = None
        # optional: (xc, gram_partial) of xyz_pregroup for these very (xyz, new_xyz, idx): the coordinates-only first layer skips its grouping pass
        self.xyz_pre = None
        # optional: compact.CompactPlan of these very idx lists -- the stack then runs on the distinct neighbours only (csrc/compact.hip)
        self.compact = None
        self.plists = None             # optional compact.PointLists of (xyz, new_xyz, idx): the gather-add backward as a segmented sum (stack.py)


def _group_src(spec, xyz, new_xyz, feats, idx):
    g = GroupSrc()
    g.xyz = xyz.data_ptr()
    g.sb, g.sn, g.sc = xyz.stride(0), xyz.stride(1), xyz.stride(2)
    g.new_xyz = new_xyz.data_ptr()
    g.feats = ptr(feats)
    g.idx = ptr(idx)
    g.N, g.S, g.K, g.D = spec.N, spec.S, spec.K, spec.D
    g.xyz_first = int(spec.xyz_first)
    return g


import os
_FUSE_RED = os.environ.get("PAPC_NO_RED") != "1"            # A/B switch for the BN-backward reduce fused into the dX epilogue
_FUSE_GMAX = os.environ.get("PAPC_NO_GMAX") != "1"          # A/B switch for the fused neighbourhood-max epilogue
_LIN_GATHER = os.environ.get("PAPC_LIN_GATHER", "1") == "1"    # first grouped layer: linear map per source point, then gather-add (lingather.hip)
_NOSTORE = os.environ.get("PAPC_NOSTORE", "1") == "1"   # the max-pooled last layer without its [M, C] output where the library has all three flavours (papc_mlp_max_nostore_ok)
_SPARSE_MAX = os.environ.get("PAPC_SPARSE_MAX", "0") == "1"   # dX of the max-pooled last layer without reading its output y (papc_mlp_bwd_dx_max_f32)
_PY_ORCH = os.environ.get("PAPC_PY_ORCH", "0") == "1"      # this module's own launch sequence instead of the library's papc_sa_mlp_fwd / _bwd (stack.py)
_XYZ1 = os.environ.get("PAPC_XYZ1", "1") == "1"             # coordinates-only first layer through its input moments, never materialised (xyz1.hip)
_XYZ_FUSE = os.environ.get("PAPC_XYZ_FUSE", "1") == "1"   # A/B switch (library orchestration only): 0 = the dX above a coordinates-only first layer is stored and read back by papc_xyz_l1_bwd_f32


# ---- W^T operands of the dX GEMMs, precomputed for several stacks in one launch -------------------------------------------------
# A stack's backward needs the transposes of its layers' weights (one papc_transpose_batch_f32 per stack).  A model that runs several
# stacks per step can transpose ALL of them in one launch before its forward (precompute_wt) and hand the resulting table to exactly
# the stack invocations of THAT forward pass (StackSpec.wt_table, kept on the autograd node).  There is no module-level state: a stack
# called without a table (a layer used on its own, a later forward after the optimiser moved the weights) transposes locally, so a
# stale transpose can never be picked up.


class WtTable(dict):
    """precompute_wt's result.  With ``lazy`` the launches are still ``pending``: :meth:`flush` issues them -- the first stack of the forward
    that runs a coordinates-only first layer through the library (stack.SharedMLPStack) lets the last of them carry that layer's finalize
    (papc_sa_mlp_xyz1_prep), and the model flushes once more behind that stack (a no-op then) before anything reads the table's tensors."""
    pending = ()

    def flush(self, l1=None):
        """``l1`` = (plan, io) of that stack, ``io.saved`` allocated.  True when the finalize rode along."""
        groups, self.pending = self.pending, ()
        lib = _lib.load()
        st = stream_ptr()
        for i, (srcs, lds, dsts, rws, cls, cps, n) in enumerate(groups):
            if l1 is not None and i == len(groups) - 1:
                check(lib.papc_sa_mlp_xyz1_prep(ctypes.byref(l1[0]), ctypes.byref(l1[1]), srcs, lds, dsts, rws, cls, cps, n, st), "papc_sa_mlp_xyz1_prep")
            else:
                check(lib.papc_transpose_batch_ld_f32(srcs, lds, dsts, rws, cls, cps, n, st), "papc_transpose_batch_ld_f32")
        return l1 is not None and bool(groups)


def precompute_wt(weights, feat_blocks=(), lazy=False):
    """weights: conv / linear weights [Cout, Cin(, 1...)] whose [Cin, Cout] transposes the coming backward passes will need.
    ``feat_blocks``: (weight [Cout, D + 3(, 1...)], xyz_first) of stacks whose first layer may run as a gather-add: the feature block -- columns
    3.. of an SSG layer's weight (coordinates first), ..D of an MSG branch's -- is made contiguous in the same launch (key
    ``("f", weight.data_ptr())``, value ``(block, xyz_first)``): the copy the stack's forward otherwise launches itself.
    ``lazy``: the launches wait for :meth:`WtTable.flush` (the caller flushes before the first stack that reads the table).
    Returns the table {weight.data_ptr(): W^T tensor, ...} to pass on as ``StackSpec.wt_table`` for this forward pass only."""
    table = WtTable()
    ok = lambda w: w.is_cuda and w.is_contiguous() and w.dtype == torch.float32      # noqa: E731
    jobs = []        # (src pointer, source row stride, destination, rows, cols, copy)
    for w in weights:
        if ok(w):
            cout = w.shape[0]
            cin = w.numel() // cout
            t = torch.empty(cin, cout, device=w.device, dtype=torch.float32)
            table[w.data_ptr()] = t
            jobs.append((w.data_ptr(), cin, t, cout, cin, 0))
    for w, xyz_first in feat_blocks:
        cout = w.shape[0]
        cin = w.numel() // cout
        if ok(w) and cin > 3:
            t = torch.empty(cout, cin - 3, device=w.device, dtype=torch.float32)
            table[("f", w.data_ptr())] = (t, bool(xyz_first))
            jobs.append((w.data_ptr() + (12 if xyz_first else 0), cin, t, cout, cin - 3, 1))
    groups = []
    for g0 in range(0, len(jobs), 8):
        grp = jobs[g0:g0 + 8]
        n = len(grp)
        srcs, dsts = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
        lds, rws, cls, cps = (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
        for i, (src, ld, t, rows, cols, cp) in enumerate(grp):
            srcs[i], lds[i], dsts[i], rws[i], cls[i], cps[i] = src, ld, t.data_ptr(), rows, cols, cp
        groups.append((srcs, lds, dsts, rws, cls, cps, n))
    table.pending = tuple(groups)
    if not lazy:
        table.flush()
    return table


def xyz_first_layer_ok(M, c1, c2, n_layers):
    """whether a coordinates-only stack of these widths takes the input-moment path of its first layer (xyz1.hip)"""
    return bool(_XYZ1 and n_layers >= 3 and _lib.load().papc_mlp_xyz_ok(M, c1, c2))


def xyz_pregroup(xyz, new_xyz, idx, out=None):
    """The weight-independent part of that path -- grouped centred coordinates xc [M, 4] and their float64 partial moments -- so a
    training loop can compute it with the sampling pyramid (layers.PointNetSetAbstraction.sample).  xyz [B,N,3] strided, new_xyz [B,S,3],
    idx [B,S,K] int32.  ``out`` = optional preallocated (xc [M,4], gram [1,16] float64)."""
    lib = _lib.load()
    B, N = xyz.shape[0], xyz.shape[1]
    S, K = idx.shape[1], idx.shape[2]
    M = B * S * K
    dev = xyz.device
    if out is None:
        out = (torch.empty(M, 4, device=dev, dtype=torch.float32), torch.empty(1, 16, device=dev, dtype=torch.float64))
    gpart = torch.empty(lib.papc_xyz_parts(M), 16, device=dev, dtype=torch.float64)
    g = GroupSrc()
    g.xyz = xyz.data_ptr()
    g.sb, g.sn, g.sc = xyz.stride(0), xyz.stride(1), xyz.stride(2)
    g.new_xyz, g.feats, g.idx = new_xyz.data_ptr(), 0, idx.data_ptr()
    g.N, g.S, g.K, g.D, g.xyz_first = N, S, K, 0, 1
    check(lib.papc_xyz_group_f32(ctypes.byref(g), B, ptr(out[0]), ptr(gpart), stream_ptr()), "papc_xyz_group_f32")
    check(lib.papc_xyz_gram_fold_f32(ptr(gpart), gpart.shape[0], ptr(out[1]), stream_ptr()), "papc_xyz_gram_fold_f32")
    return out


class SharedMLPMax(torch.autograd.Function):
    """out[g, :] = max_{k<K} relu(bn_L(conv_L(... relu(bn_1(conv_1(rows)))...)))   with rows gathered on the fly.

    apply(spec, bn_buffers, xyz, new_xyz, feats, idx, x_rows, w1, b1, gamma1, beta1, w2, ...)
      x_rows   None, or plain input rows [M, Cin] (then xyz/new_xyz/feats/idx are ignored: PFNLayer)
      xyz      [B,N,3] any strides        new_xyz [B,S,3] contiguous
      feats    [B,N,D] contiguous or None idx     [B,S,K] int32 or None (identity: S=1, K=N)
      w_l      [C_l, C_{l-1}] (conv weight, trailing 1x1 dims dropped); b_l, gamma_l, beta_l [C_l]
      bn_buffers: list of (running_mean, running_var) per layer (updated in place) or None
    returns [B*S, C_L]   (spec.pool=False: [M, C_L], every row's activation)
    """

    @staticmethod
    def forward(ctx, spec, bn_buffers, xyz, new_xyz, feats, idx, x_rows, *params):
        lib = _lib.load()
        st = stream_ptr()
        dev = params[0].device
        L = len(params) // 4
        M = spec.M
        parts = lib.papc_mlp_gemm_parts(M)
        plain = x_rows is not None
        grp = None if plain else _group_src(spec, xyz, new_xyz, feats, idx)
        ys, consts = [], []
        prev_y, prev_sc, prev_sh = None, None, None
        cin = x_rows.shape[1] if plain else spec.D + 3
        cin0 = cin
        ev = spec.eval_bn
        assert not ev or bn_buffers is not None, "eval_bn needs the running statistics"
        lin0 = (_LIN_GATHER and not ev and not plain and idx is not None and feats is not None and L >= 2 and spec.D % 4 == 0 and spec.D >= 16
                and params[0].shape[0] % 4 == 0 and params[0].shape[0] <= 256 and feats.is_contiguous())
        # coordinates-only first layer (D = 0): its [M, C1] output is never stored -- BN statistics from the inputs' second moments, the
        # layer folded into the second layer's operand (xyz1.hip)
        xyz1 = (not ev and not plain and idx is not None and feats is None and spec.D == 0
                and xyz_first_layer_ok(M, params[0].shape[0], params[4].shape[0] if L >= 2 else 0, L))
        xc = wf = gram = None
        # compacted stack: distinct neighbours only, a weight on each group's first row (compact.py); the row count is a device-side number
        cp = spec.compact if (lin0 and spec.pool and spec.compact is not None) else None
        if cp is not None:
            from . import compact as _cpm
            if not _cpm.stack_ok(M, spec.K, [params[4 * l].shape[0] for l in range(L)]):
                cp = None
        R_c = lib.papc_compact_corr_parts() if cp is not None else 0     # extra statistics rows: the copies' share
        if cp is not None:
            grp.cidx, grp.seg_grp, grp.rows_dev = cp.cidx.data_ptr(), cp.seg_grp.data_ptr(), cp.rows.data_ptr()
        for l in range(L):
            w, b, gamma, beta = params[4 * l: 4 * l + 4]
            cout = w.shape[0]
            w2 = w.reshape(cout, cin)
            assert w2.is_contiguous()
            stats = None if ev else torch.empty(parts + R_c, 2, cout, device=dev, dtype=torch.float32)
            parts_l = parts
            gm_ref = None
            if cp is None and l == L - 1 and spec.pool and _FUSE_GMAX and not ev and lib.papc_mlp_gemm_gmax_ok(M, cout, spec.K):
                # last layer: the neighbourhood max is reduced in the GEMM epilogue (per-group max/min of the raw output)
                G_ = M // spec.K
                gbuf_f = torch.empty(2, G_, cout, device=dev, dtype=torch.float32)
                gbuf_i = torch.empty(2, G_, cout, device=dev, dtype=torch.int32)
                gm = GroupMax()
                gm.gmax, gm.gmin = gbuf_f[0].data_ptr(), gbuf_f[1].data_ptr()
                gm.amax, gm.amin = gbuf_i[0].data_ptr(), gbuf_i[1].data_ptr()
                gm.K = spec.K
                gm_ref = ctypes.byref(gm)
            if (gm_ref is not None and _NOSTORE and L >= 2 and l == L - 1 and prev_y is not None and not (l == 1 and xyz1)
                    and lib.papc_mlp_max_nostore_ok(M, cin, cout, spec.K)):
                y = None                           # the pooled layer's own output is never stored: extrema + statistics forward, input sums backward
            else:
                y = None if (l == 0 and xyz1) else torch.empty(M, cout, device=dev, dtype=torch.float32)
            if l == 0 and xyz1:
                y = stats = None
                nparts = 1                         # (the moments arrive folded: xyz_pregroup)
                if spec.xyz_pre is not None:       # grouped with the sampling pyramid (possibly on another stream, one step ahead)
                    xc, gpart = spec.xyz_pre
                    assert tuple(xc.shape) == (M, 4) and tuple(gpart.shape) == (1, 16)
                else:
                    xc, gpart = xyz_pregroup(xyz, new_xyz, idx)
                cst = torch.empty(4, cout, device=dev, dtype=torch.float32)
                wf = torch.empty(cout, 4, device=dev, dtype=torch.float32)
                gram = torch.empty(16, device=dev, dtype=torch.float64)
                rm, rv = (bn_buffers[l] if bn_buffers is not None else (None, None))
                check(lib.papc_xyz_l1_finalize_f32(ptr(gpart), nparts, M, ptr(w2), cin, 0, ptr(b), ptr(gamma), ptr(beta), spec.eps, spec.momentum,
                                                   cout, *cst_ptrs(cst), ptr(rm), ptr(rv), ptr(wf), ptr(gram), st), "papc_xyz_l1_finalize_f32")
                ys.append(None)
                consts.append(cst)
                prev_y, prev_sc, prev_sh = None, cst[2], cst[3]
                cin = cout
                continue
            if l == 1 and xyz1:
                check(lib.papc_mlp_gemm_f32(A_XYZ, ptr(xc), 4, None, ptr(wf), None, ptr(w2), ptr(b), M, cin, cout,
                                            ptr(y), ptr(stats), gm_ref, st), "papc_mlp_gemm_f32")
            elif l == 0 and plain:
                check(lib.papc_mlp_gemm_f32(A_PLAIN, ptr(x_rows), cin, None, None, None, ptr(w2), ptr(b), M, cin, cout,
                                            ptr(y), ptr(stats), gm_ref, st), "papc_mlp_gemm_f32")
            elif l == 0 and lin0:
                # W_f feats_j depends on the source point only: one [B*N, D] x [D, cout] product (the row GEMM kernel, plain input, no
                # bias / statistics) on the feature block of the weight, then a streaming gather-add
                fcol0 = 3 if spec.xyz_first else 0
                wf = torch.empty(cout, spec.D, device=dev, dtype=torch.float32)
                check(lib.papc_copy2d_f32(w2.data_ptr() + 4 * fcol0, cin, ptr(wf), spec.D, cout, spec.D, 0, st), "papc_copy2d_f32")
                BN_ = spec.B * spec.N
                P = torch.empty(BN_, cout, device=dev, dtype=torch.float32)
                check(lib.papc_mlp_gemm_f32(A_PLAIN, ptr(feats), spec.D, None, None, None, ptr(wf), None, BN_, spec.D, cout, ptr(P), None,
                                            None, st), "papc_mlp_gemm_f32")
                parts_l = lib.papc_lingather_parts(M)
                stats = torch.empty(parts_l + R_c, 2, cout, device=dev, dtype=torch.float32)
                check(lib.papc_lingather_fwd_f32(ptr(P), ctypes.byref(grp), spec.B, ptr(w2), cin, 0 if spec.xyz_first else spec.D,
                                                 ptr(b), cout, ptr(y), ptr(stats), st), "papc_lingather_fwd_f32")
            elif l == 0:
                check(lib.papc_mlp_gemm_f32(A_GROUP, None, 0, ctypes.byref(grp), None, None, ptr(w2), ptr(b), M, cin, cout,
                                            ptr(y), ptr(stats), gm_ref, st), "papc_mlp_gemm_f32")
            elif cp is not None:
                check(lib.papc_mlp_gemm_rows_f32(A_BNRELU, ptr(prev_y), cin, None, ptr(prev_sc), ptr(prev_sh), ptr(w2), ptr(b), M, cin,
                                                 cout, ptr(y), ptr(stats), None, cp.rows.data_ptr(), st), "papc_mlp_gemm_rows_f32")
            else:
                check(lib.papc_mlp_gemm_f32(A_BNRELU, ptr(prev_y), cin, None, ptr(prev_sc), ptr(prev_sh), ptr(w2), ptr(b), M, cin,
                                            cout, ptr(y), ptr(stats), gm_ref, st), "papc_mlp_gemm_f32")
            if cp is not None:      # what the copies add to this layer's statistics: R_c extra partial rows behind the kernel's own
                check(lib.papc_bn_stats_corr_f32(ptr(y), cout, cp.start.data_ptr(), cp.coef.data_ptr(), cp.G,
                                                 stats.data_ptr() + 4 * parts_l * 2 * cout, st), "papc_bn_stats_corr_f32")
                parts_l += R_c
            cst = torch.empty(4, cout, device=dev, dtype=torch.float32)  # mean, invstd, scale, shift
            rm, rv = (bn_buffers[l] if bn_buffers is not None else (None, None))
            if ev:
                check(lib.papc_bn_eval_consts_f32(ptr(rm), ptr(rv), ptr(gamma), ptr(beta), spec.eps, cout, *cst_ptrs(cst), st), "papc_bn_eval_consts_f32")
            else:
                check(lib.papc_bn_finalize_f32(ptr(stats), parts_l, M, cout, ptr(gamma), ptr(beta), spec.eps, spec.momentum, *cst_ptrs(cst),
                                               ptr(rm), ptr(rv), st), "papc_bn_finalize_f32")
            ys.append(y)
            consts.append(cst)
            prev_y, prev_sc, prev_sh = y, cst[2], cst[3]
            cin = cout
        G = spec.B * spec.S
        argmax = None
        if not spec.pool:
            out = torch.empty(M, cin, device=dev, dtype=torch.float32)
            check(lib.papc_bn_relu_f32(ptr(prev_y), ptr(prev_sc), ptr(prev_sh), M, cin, ptr(out), st), "papc_bn_relu_f32")
        else:
            out = torch.empty(G, cin, device=dev, dtype=torch.float32)
            argmax = torch.empty(G, cin, device=dev, dtype=torch.int32)
        ysel_c = None
        if not spec.pool:
            pass
        elif cp is not None:            # ragged groups: the max runs over each group's physical rows; argmax = absolute row
            ysel_c = torch.empty(G, cin, device=dev, dtype=torch.float32)
            check(lib.papc_bn_relu_max_seg_f32(ptr(prev_y), cin, cp.start.data_ptr(), ptr(prev_sc), ptr(prev_sh), G, ptr(out), ptr(argmax),
                                               ptr(ysel_c), st), "papc_bn_relu_max_seg_f32")
        elif gm_ref is not None:
            check(lib.papc_bn_select_max_f32(gbuf_f[0].data_ptr(), gbuf_f[1].data_ptr(), gbuf_i[0].data_ptr(), gbuf_i[1].data_ptr(),
                                             ptr(prev_sc), ptr(prev_sh), G, cin, ptr(out), ptr(argmax), st), "papc_bn_select_max_f32")
        else:
            check(lib.papc_bn_relu_max_f32(ptr(prev_y), ptr(prev_sc), ptr(prev_sh), G, spec.K, cin, ptr(out), ptr(argmax), st),
                  "papc_bn_relu_max_f32")
        ctx.spec = spec
        ctx.L = L
        ctx.wt_table = spec.wt_table
        ctx.feats_needs_grad = feats is not None and feats.requires_grad and not spec.cut_gather_grad
        ctx.x_needs_grad = plain and x_rows.requires_grad
        ctx.cin0 = cin0
        ctx.lin0 = lin0
        ctx.xyz1 = xyz1
        ctx.nostore = spec.pool and L >= 1 and ys[L - 1] is None and not (xyz1 and L == 1)
        ysel = gbuf_f[0] if (spec.pool and gm_ref is not None) else ysel_c   # raw y at the argmax (left in gmax by select_max)
        ctx.compact = cp
        if xyz1:
            ys[0] = xc                 # (slot of the first layer's output, which does not exist: the grouped coordinates instead)
            consts = consts + [wf, gram]
        ctx.save_for_backward(xyz, new_xyz, feats, idx, x_rows, argmax, ysel, *params, *ys, *consts)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        st = stream_ptr()
        spec, L = ctx.spec, ctx.L
        saved = ctx.saved_tensors
        xyz, new_xyz, feats, idx, x_rows, argmax, ysel = saved[:7]
        params = saved[7:7 + 4 * L]
        ys = saved[7 + 4 * L: 7 + 5 * L]
        consts = saved[7 + 5 * L: 7 + 6 * L]
        xyz1 = ctx.xyz1
        xc = wf = gram = None
        if xyz1:
            xc, (wf, gram) = ys[0], saved[7 + 6 * L: 7 + 6 * L + 2]
        plain = x_rows is not None
        dev = gout.device
        M = spec.M
        gout = gout.contiguous().float()
        grp = None if plain else _group_src(spec, xyz, new_xyz, feats, idx)
        cp = ctx.compact
        if cp is not None:
            grp.cidx, grp.seg_grp, grp.rows_dev = cp.cidx.data_ptr(), cp.seg_grp.data_ptr(), cp.rows.data_ptr()
        grads = [None] * (4 * L)
        reduce_jobs = []   # (DwPartials, (dW pointer, db pointer, accumulate)): see the dW section
        grad_feats = None
        grad_x = None
        dz = None
        fused_red = None
        gemm_parts = lib.papc_mlp_gemm_parts(M)
        # W^T operands of every dX GEMM of the stack: one batched transpose launch
        need_wt = [l for l in range(L) if l > 0 or (plain and ctx.x_needs_grad) or ((not plain) and ctx.feats_needs_grad)]
        # last layer under the max: its dX can be formed from the [G, C] max-backward arrays and the layer's INPUT, without its output
        cL, cLi = params[4 * (L - 1)].shape[0], (params[4 * (L - 2)].shape[0] if L > 1 else 0)
        sparse_max = ctx.nostore or (_SPARSE_MAX and spec.pool and L > 1 and ysel is not None and M >= 32768 and cL % 16 == 0 and cLi % 4 == 0
                                     and cL + cLi <= 512)
        max_prep = None     # (psel, wcat, hbias, e) of the sparse-max backward, shared by its dW and dX
        if sparse_max:
            need_wt.remove(L - 1)
        if ctx.lin0 and 0 in need_wt:
            need_wt.remove(0)
        wts = {}
        if ctx.wt_table is not None:       # transposes handed over for this very forward pass (precompute_wt)
            for l in list(need_wt):
                t = ctx.wt_table.get(params[4 * l].data_ptr())
                cin_l = ctx.cin0 if l == 0 else params[4 * (l - 1)].shape[0]
                if t is not None and tuple(t.shape) == (cin_l, params[4 * l].shape[0]):
                    wts[l] = t
                    need_wt.remove(l)
        for g0 in range(0, len(need_wt), 8):
            grp_l = need_wt[g0:g0 + 8]
            n = len(grp_l)
            srcs, dsts, rws, cls = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
            for i, l in enumerate(grp_l):
                w = params[4 * l]
                cout = w.shape[0]
                cin = ctx.cin0 if l == 0 else params[4 * (l - 1)].shape[0]
                assert w.is_contiguous()
                wts[l] = torch.empty(cin, cout, device=dev, dtype=torch.float32)
                srcs[i], dsts[i], rws[i], cls[i] = w.data_ptr(), wts[l].data_ptr(), cout, cin
            check(lib.papc_transpose_batch_f32(srcs, dsts, rws, cls, n, st), "papc_transpose_batch_f32")
        for l in range(L - 1, -1, -1):
            w = params[4 * l]
            cout = w.shape[0]
            cin = ctx.cin0 if l == 0 else params[4 * (l - 1)].shape[0]
            cst = consts[l]
            c12 = torch.empty(2, cout, device=dev, dtype=torch.float32)
            s = LayerSlots(spec.grad_targets, l, w, spec.eval_bn, xyz_first_layer=(l == 0 and xyz1))
            grads[4 * l: 4 * l + 4] = s.grads
            dy = BwdDy()
            if cp is not None:      # multiplicity weights, ragged groups, device-side row count
                dy.wrow, dy.seg_grp, dy.rows_dev = cp.wrow.data_ptr(), cp.seg_grp.data_ptr(), cp.rows.data_ptr()
            if l == L - 1 and not spec.pool:
                dy.dz_mode, dy.dz, dy.gout, dy.argmax, dy.K = DZ_DENSE, gout.data_ptr(), None, None, 1
            elif l == L - 1:
                dy.dz_mode, dy.dz, dy.gout, dy.argmax, dy.K = DZ_MAX, None, gout.data_ptr(), argmax.data_ptr(), spec.K
            else:
                dy.dz_mode, dy.dz, dy.gout, dy.argmax, dy.K = DZ_DENSE, dz.data_ptr(), None, None, 1
            if l == 0 and xyz1:
                # the whole backward of the coordinates-only layer from one pass over dz and the inputs' moments: p = dz [a > 0] summed
                # against the coordinates, then closed forms for dgamma / dbeta / dW (no y, no BN-backward sums from the layer above)
                nbp = lib.papc_xyz_bwd_parts(M)
                bpart = torch.empty(nbp, cout, 4, device=dev, dtype=torch.float32)
                check(lib.papc_xyz_l1_bwd_f32(ptr(dz), ptr(xc), ptr(wf), M, cout, ptr(bpart), st), "papc_xyz_l1_bwd_f32")
                mean, invstd, scale, _ = cst_ptrs(cst)
                check(lib.papc_xyz_l1_bwd_finalize_f32(ptr(bpart), nbp, M, cout, ptr(gram), ptr(w), cin, 0, ptr(params[1]), mean, invstd, scale,
                                                       s.dgamma_p, s.dbeta_p, s.dw_p, s.acc_w, st), "papc_xyz_l1_bwd_finalize_f32")
                s.zero_db()
                break
            dy.set_bn(ys[l], cst, c12)
            # (sum p, sum p*xhat): a separate pass, unless the dX kernel of layer l+1 already produced them; under the sparse max the same
            # pass also writes the sparse operand of this layer's dX / dW
            psel = torch.empty(M // spec.K, cout, device=dev, dtype=torch.float32) if (sparse_max and l == L - 1) else None
            bn_bwd_sums(dy, M, cout, c12, s.dgamma_p, s.dbeta_p, s.acc_gb, spec.eval_bn, dz=ptr(ysel) if dy.dz_mode == DZ_MAX else None,
                        red=fused_red, psel=psel)
            if l == 0 and ctx.lin0:
                # G[j] = sum of the dY rows that gathered point j (+ the xyz columns of dW, streamed); the D-wide products run on B*N rows
                BN_ = spec.B * spec.N
                parts_l = lib.papc_lingather_parts(M)
                dwx_part = torch.empty(parts_l, cout * 3, device=dev, dtype=torch.float32)
                Gs = _lib.zeros((BN_, cout), dev)
                check(lib.papc_lingather_bwd_f32(ctypes.byref(dy), ctypes.byref(grp), spec.B, cout, ptr(Gs), ptr(dwx_part), st),
                      "papc_lingather_bwd_f32")
                # the gradient lands in ONE [cout, cin] tensor -- the parameter's .grad view (accumulate) or a fresh one: the
                # coordinate block and the feature block are summed straight into their column ranges (no concat, no add)
                fcol0, xcol0 = (3, 0) if spec.xyz_first else (0, spec.D)
                check(lib.papc_reduce_partials_strided_f32(ptr(dwx_part), parts_l, cout * 3, cout, 3, s.dw_p + 4 * xcol0, cin, s.acc_w, st),
                      "papc_reduce_partials_strided_f32")
                # dW_f = G^T feats on the library's own dW kernel: G plays dY with the identity constants (dY = dz); chunks of >= 64 rows
                dyg = BwdDy()
                dyg.dz_mode, dyg.dz, dyg.gout, dyg.argmax, dyg.K = DZ_DENSE, Gs.data_ptr(), None, None, 1
                identity_bn(dyg, Gs, cout, dev)
                DwPartials(dyg, A_PLAIN, ptr(feats), spec.D, None, None, None, BN_, spec.D, cout, dev, min_rows=64).fold_cols(
                    s.dw_p + 4 * fcol0, cin, s.acc_w)
                s.zero_db()
                if ctx.feats_needs_grad:
                    # grad_feats = G W_f: the same row GEMM with the transposed feature block as its weight
                    wt_full = ctx.wt_table.get(w.data_ptr()) if ctx.wt_table is not None else None
                    if wt_full is not None and tuple(wt_full.shape) == (cin, cout):
                        wft = wt_full[fcol0:fcol0 + spec.D]     # rows of the precomputed W^T [cin, cout]: the feature block, contiguous
                    else:
                        wft = torch.empty(spec.D, cout, device=dev, dtype=torch.float32)
                        check(lib.papc_copy2d_f32(w.data_ptr() + 4 * fcol0, cin, ptr(wft), cout, cout, spec.D, 1, st), "papc_copy2d_f32")
                    grad_feats = torch.empty(spec.B, spec.N, spec.D, device=dev, dtype=torch.float32)
                    check(lib.papc_mlp_gemm_f32(A_PLAIN, ptr(Gs), cout, None, None, None, ptr(wft), None, BN_, cout, spec.D, ptr(grad_feats),
                                                None, None, st), "papc_mlp_gemm_f32")
                break
            if sparse_max and l == L - 1:
                G = M // spec.K
                wcat = torch.empty(cin, cout + cin, device=dev, dtype=torch.float32)
                hb = torch.empty(cin, device=dev, dtype=torch.float32)
                eq = torch.empty(2, cout, device=dev, dtype=torch.float32)
                check(lib.papc_bn_max_prep_f32(None, None, cst[2].data_ptr(), cst[3].data_ptr(), cst[0].data_ptr(),
                                               cst[1].data_ptr(), c12[0].data_ptr(), c12[1].data_ptr(), ptr(w), ptr(params[4 * l + 1]),
                                               G, cout, cin, None, ptr(wcat), ptr(hb), eq[0].data_ptr(), eq[1].data_ptr(), st),
                      "papc_bn_max_prep_f32")      # (psel: written by the reduction above)
                max_prep = (psel, wcat, hb, eq)
            # ---- dW, db
            if ctx.nostore and l == L - 1:
                # no stored output: T = P'^T A, the Gram matrix of the input rows and their column sums in one pass, closed form for dW
                pc = consts[l - 1]
                ws = torch.empty(lib.papc_mlp_bwd_dw_max_ws_floats(M, cin, cout), device=dev, dtype=torch.float32)
                check(lib.papc_mlp_bwd_dw_max_f32(ptr(max_prep[0]), ptr(argmax), spec.K, ys[l - 1].data_ptr(), pc[2].data_ptr(), pc[3].data_ptr(),
                                                  ptr(w), max_prep[3][0].data_ptr(), cst[2].data_ptr(), c12[0].data_ptr(), M, cin, cout,
                                                  ptr(ws), s.dw_p, s.acc_w, st), "papc_mlp_bwd_dw_max_f32")
                s.zero_db()
            x1 = xyz1 and l == 1             # the input of this layer is the recomputed activation of the coordinates-only first layer
            if not (ctx.nostore and l == L - 1):
                if l == 0 and plain:
                    a_op = (A_PLAIN, ptr(x_rows), cin, None, None, None)
                elif l == 0:
                    a_op = (A_GROUP, None, 0, ctypes.byref(grp), None, None)
                elif x1:
                    a_op = (A_XYZ, ptr(xc), 4, None, ptr(wf), None)
                else:
                    pc = consts[l - 1]
                    a_op = (A_BNRELU, ys[l - 1].data_ptr(), cin, None, pc[2].data_ptr(), pc[3].data_ptr())
                part = DwPartials(dy, *a_op, M, cin, cout, dev)
                # the partials of all layers are folded in ONE launch once the stack's last dW kernel is enqueued (papc_reduce_partials_batch_f32)
                if s.acc_w or not spec.eval_bn:
                    reduce_jobs.append((part, (s.dw_p, s.db_p, s.acc_w)))
                else:                     # no batch-mean term removes the bias direction: db = sum_m dy = scale * sum_m p (tiny [C] op)
                    part.fold(s.dw_p, s.db_p, 0)
                    grads[4 * l + 1] = cst[2] * grads[4 * l + 3]
            # ---- dX
            fused_red = None
            if l > 0:
                wt = wts.get(l)
                dz_prev = torch.empty(M, cin, device=dev, dtype=torch.float32)
                # the dX kernel also accumulates layer l-1's BN-backward reductions over the dz it produces
                nr_ref = None
                if _FUSE_RED and not x1:     # (x1: the layer below takes its BN-backward sums from its own pass over dz, xyz1.hip)
                    fused_red = torch.empty(gemm_parts, 2, cin, device=dev, dtype=torch.float32)
                    nr = BwdRed()
                    nr.y = ys[l - 1].data_ptr()
                    nr.mean, nr.invstd, nr.scale, nr.shift = cst_ptrs(consts[l - 1])
                    nr.red_partial = fused_red.data_ptr()
                    nr_ref = ctypes.byref(nr)
                if sparse_max and l == L - 1:
                    psel, wcat, hb, _ = max_prep
                    pc = consts[l - 1]
                    check(lib.papc_mlp_bwd_dx_max_f32(ptr(psel), ptr(argmax), spec.K, ys[l - 1].data_ptr(), cin, pc[2].data_ptr(),
                                                      pc[3].data_ptr(), ptr(wcat), ptr(hb), M, cin, cout, ptr(dz_prev), nr_ref, st),
                          "papc_mlp_bwd_dx_max_f32")
                else:
                    check(lib.papc_mlp_bwd_dx_f32(ctypes.byref(dy), ptr(wt), M, cin, cout, ptr(dz_prev), None, nr_ref, st),
                          "papc_mlp_bwd_dx_f32")
                dz = dz_prev
            elif plain and ctx.x_needs_grad:
                wt = wts[l]
                grad_x = torch.empty(M, cin, device=dev, dtype=torch.float32)
                check(lib.papc_mlp_bwd_dx_f32(ctypes.byref(dy), ptr(wt), M, cin, cout, ptr(grad_x), None, None, st), "papc_mlp_bwd_dx_f32")
            elif (not plain) and ctx.feats_needs_grad:
                wt = wts[l]
                grad_feats = _lib.zeros((spec.B, spec.N, spec.D), dev)
                sc = ScatterDst()
                sc.grad_feats, sc.idx = grad_feats.data_ptr(), ptr(idx)
                sc.N, sc.S, sc.K, sc.D = spec.N, spec.S, spec.K, spec.D
                sc.col0 = 3 if spec.xyz_first else 0
                check(lib.papc_mlp_bwd_dx_f32(ctypes.byref(dy), ptr(wt), M, cin, cout, None, ctypes.byref(sc), None, st), "papc_mlp_bwd_dx_f32")
        launch_batched(ReduceJob, [p.job(*out) for p, out in reduce_jobs], lib.papc_reduce_partials_batch_f32, "papc_reduce_partials_batch_f32")
        return (None, None, None, None, grad_feats, None, grad_x) + tuple(grads)


def shared_mlp_max(spec, bn_buffers, xyz, new_xyz, feats, idx, params, x_rows=None):
    # re-evaluated on every forward: a cached list would go stale when the optimizer replaces the .grad tensors
    # (e.g. zero_grad(set_to_none=True)) and gradients would silently land in orphaned buffers
    spec.grad_targets = grad_targets_of(params) if (torch.is_grad_enabled() and not spec.eval_bn) else None
    if _PY_ORCH or _SPARSE_MAX:       # the call sequences spelled out in Python (A/B against the library's own orchestration, csrc/sa_mlp.hip)
        from . import smallm
        if smallm.eligible(spec, xyz, feats, idx, x_rows, params):      # few rows, groups of 128 (group_all layers): csrc/smallm.hip
            return smallm.PlanesMLPMax.apply(spec, bn_buffers, xyz, new_xyz, feats, idx, x_rows, *params)
        return SharedMLPMax.apply(spec, bn_buffers, xyz, new_xyz, feats, idx, x_rows, *params)
    from .stack import SharedMLPStack
    return SharedMLPStack.apply(spec, bn_buffers, xyz, new_xyz, feats, idx, x_rows, *params)
