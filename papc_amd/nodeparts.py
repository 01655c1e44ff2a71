"""The host-side rules the autograd nodes share, each written once: where a gradient goes (in place into ``.grad`` or back through
autograd), the identity BatchNorm constants that let a Linear without a norm ride the BN-aware kernels, the BN-backward sums, the dW
partial buffer and "at most 8 jobs per launch".  A leaf module: it imports only ``_lib``, ``ctypes`` and ``torch``.
"""
import ctypes

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

DZ_MAX = 1               # papc_bwd_dy.dz_mode under the max (PAPC_DZ_MAX)


# ---- gradient targets ---------------------------------------------------------------------------------------------------------------

def grad_targets_of(params):
    """Per parameter: its .grad tensor when the parameter opted in to in-place accumulation (a view of distributed.FlatParams.grad),
    else None -- or None altogether when no parameter did.  With a target the backward adds the gradient in place (one fused accumulate
    in the reduce kernels) and hands autograd ``None`` for it: no per-parameter AccumulateGrad add kernels.  Entries that are not
    opted-in leaf Parameters (e.g. the zero-padded view of a first conv weight, layers._pad_features) go back through autograd as usual."""
    tg = []
    for p in params:
        g = None
        # explicit opt-in (distributed.FlatParams marks its parameters): writing .grad behind autograd's back skips AccumulateGrad
        # hooks, so torch's DistributedDataParallel, post-accumulate hooks, torch.autograd.grad() and checkpoint recomputation would
        # miss or double-count these gradients -- a parameter that merely HAS a .grad (second step of any plain optimizer loop) does
        # not qualify
        if isinstance(p, torch.nn.Parameter) and getattr(p, "_papc_inplace_grad", False):
            g = p.grad
            if not (p.requires_grad and g is not None and g.is_contiguous() and g.dtype == torch.float32 and g.shape == p.shape):
                g = None
        tg.append(g)
    return tg if any(t is not None for t in tg) else None


class LayerSlots:
    """Where the four gradients (w, b, gamma, beta) of one conv + norm layer go: ``dw_p, db_p, dgamma_p, dbeta_p`` to hand the kernels
    (``db_p`` None: nothing to write), the accumulate flags ``acc_w`` (dW, db) and ``acc_gb`` (dgamma, dbeta), and ``grads``, the four
    entries for autograd (None where the gradient went in place)."""

    def __init__(self, targets, l, w, eval_bn, xyz_first_layer=False):
        """``targets``: grad_targets_of() of the stack's parameters (or None), ``l``: the layer, ``w`` its weight [cout, cin(, 1...)];
        ``xyz_first_layer``: the coordinates-only first layer, which takes ONE accumulate flag for dW, dgamma and dbeta."""
        cout = w.shape[0]
        new = lambda *shape: torch.empty(*shape, device=w.device, dtype=torch.float32)      # noqa: E731
        tgt = targets[4 * l: 4 * l + 4] if targets is not None else (None,) * 4
        inplace = all(t is not None for t in tgt)
        # the norm's two vectors can go in place on their own (a layer whose conv weight is a padded view keeps them off autograd)
        gb_inplace = tgt[2] is not None and tgt[3] is not None and not eval_bn
        self.grads = [None] * 4
        self.db = None
        if inplace:          # accumulate straight into the parameters' .grad (flat-bucket views): no autograd add kernels
            self.dw_p, self.db_p, self.acc_w = tgt[0].data_ptr(), tgt[1].data_ptr(), 1
        else:
            dw = new(cout, w.numel() // cout)
            self.grads[0] = dw.reshape(w.shape)
            self.dw_p, self.db_p, self.acc_w = dw.data_ptr(), None, 0
            if tgt[1] is None or eval_bn:      # (else a bias under a train-mode BN: gradient exactly 0 -- nothing to add in place)
                self.db = self.grads[1] = new(cout)
                self.db_p = self.db.data_ptr()
        if gb_inplace and (inplace or not xyz_first_layer):
            self.dgamma_p, self.dbeta_p, self.acc_gb = tgt[2].data_ptr(), tgt[3].data_ptr(), 1
        else:
            dgb = new(2, cout)
            self.grads[2], self.grads[3] = dgb[0], dgb[1]
            self.dgamma_p, self.dbeta_p, self.acc_gb = dgb[0].data_ptr(), dgb[1].data_ptr(), 0

    def zero_db(self):
        """for a kernel that never writes db (a bias feeding a train-mode BN has gradient exactly 0): fill the fresh tensor, if there is one"""
        if self.db is not None:
            check(_lib.load().papc_fill_f32(self.db.data_ptr(), self.db.numel(), 0.0, stream_ptr()), "papc_fill_f32")


def all_or_none(targets, shapes, dev):
    """The single-kernel nodes take one accumulate flag: every gradient in place or none (a partial target set counts as none).
    -> (tensors to write, accumulate flag, the entries for autograd)"""
    if targets is not None and all(t is not None for t in targets):
        return list(targets), 1, (None,) * len(targets)
    fresh = [torch.empty(s, device=dev, dtype=torch.float32) for s in shapes]
    return fresh, 0, tuple(fresh)


# ---- BN-backward: identity constants, the two sums --------------------------------------------------------------------------------------

def identity_bn(dy, y, C, dev, relu=False):
    """Fill ``dy`` (a BwdDy) so that the BN-aware kernels serve a Linear WITHOUT a norm: mean 0, invstd 1, scale 1, c1 = c2 = 0 and
    shift 1e30 (the ReLU mask is always on: dY = dz) or, ``relu``, shift 0 (dY = dz [y > 0]).  Cached vectors, safe under capture."""
    one, zero = _lib.const_vec(1.0, C, dev), _lib.const_vec(0.0, C, dev)
    shift = zero if relu else _lib.const_vec(1e30, C, dev)
    dy.y = ptr(y)
    dy.mean, dy.invstd, dy.scale, dy.shift = zero.data_ptr(), one.data_ptr(), one.data_ptr(), shift.data_ptr()
    dy.c1, dy.c2 = zero.data_ptr(), zero.data_ptr()


def bn_bwd_sums(dy, M, C, c12, dgamma_p, dbeta_p, accumulate=0, eval_bn=False, dz=None, red=None, psel=None):
    """(sum p, sum p * xhat) over the M rows of the layer ``dy`` (a BwdDy) describes, then dgamma, dbeta and the constants c1, c2 into
    ``c12`` [2, C]: papc_bn_bwd_reduce_f32 over min(512, ceil(M / 128)) partial rows (sa_mlp.hip: the same count) and
    papc_bn_bwd_finalize_f32 (flag bits: 1 accumulate into dgamma / dbeta, 2 eval-mode norm).
    ``red``: the partial rows [parts, 2, C] a producer already wrote (no reduce launch); ``dz``: the values to read instead of dy.dz
    (under the max: y at the argmax); ``psel`` [G, C]: the reduce that also writes the sparse operand of the max layer's dX / dW."""
    lib, st = _lib.load(), stream_ptr()
    if red is None:
        red = torch.empty(min(512, (M + 127) // 128), 2, C, device=c12.device, dtype=torch.float32)
        if psel is not None:
            check(lib.papc_bn_bwd_reduce_max_f32(dz, dy.gout, dy.K, dy.mean, dy.invstd, dy.scale, dy.shift, M, C, red.shape[0], ptr(red),
                                                 ptr(psel), st), "papc_bn_bwd_reduce_max_f32")
        else:
            check(lib.papc_bn_bwd_reduce_f32(dy.dz_mode, dy.dz if dz is None else dz, dy.gout, dy.argmax, dy.K, dy.y, dy.mean, dy.invstd,
                                             dy.scale, dy.shift, M, C, red.shape[0], ptr(red), st), "papc_bn_bwd_reduce_f32")
    check(lib.papc_bn_bwd_finalize_f32(ptr(red), red.shape[0], M, C, dgamma_p, dbeta_p, c12[0].data_ptr(), c12[1].data_ptr(),
                                       (1 if accumulate else 0) | (2 if eval_bn else 0), st), "papc_bn_bwd_finalize_f32")


# ---- the dW partial buffer -------------------------------------------------------------------------------------------------------------

def _dw_rows_per_chunk(M, cout, cin, min_rows=256):
    """Row-chunk size for the dW kernel: ONE residency wave of workgroups (256 CUs x 2 per CU = 512) in total, so
    no tail round; chunks of >= 256 rows -- >= 64 for the gather-add layer's dW_f over the B N source points (sa_mlp.hip::dw_rows_per_chunk:
    the same rule, bit for bit the same partial sums)."""
    wide = 128 < cin <= 160
    tiles = ((cout + 127) // 128) * (1 if wide else (cin + 127) // 128)
    want = max(1, 512 // tiles)
    rpc = (M + want - 1) // want
    rpc = max(min_rows, ((rpc + 63) // 64) * 64)
    return rpc


class DwPartials:
    """dW = dY^T . A of one layer as per-chunk partial sums: picks the rows per chunk (the kernel's own preference where it has one,
    papc_mlp_bwd_dw_chunk_hint, else _dw_rows_per_chunk), allocates the [n_chunks, cout * cin + cout] buffer -- a chunk's row is
    [dW (cout * cin) | db (cout)] -- and launches papc_mlp_bwd_dw_f32.  ``a_mode, x, ldx, grp, a1, a2``: the kernel's A operand."""

    def __init__(self, dy, a_mode, x, ldx, grp, a1, a2, M, cin, cout, dev, min_rows=256):
        lib = _lib.load()
        rpc = lib.papc_mlp_bwd_dw_chunk_hint(M, cin, cout, a_mode, dy.dz_mode, dy.K if dy.dz_mode == DZ_MAX else 0)
        if rpc <= 0:
            rpc = _dw_rows_per_chunk(M, cout, cin, min_rows)
        self.n_chunks, self.cout, self.cin, self.ld = (M + rpc - 1) // rpc, cout, cin, cout * cin + cout
        self.part = torch.empty(self.n_chunks, self.ld, device=dev, dtype=torch.float32)
        check(lib.papc_mlp_bwd_dw_f32(ctypes.byref(dy), a_mode, x, ldx, grp, a1, a2, M, cin, cout, rpc, self.part.data_ptr(),
                                      self.part.data_ptr() + 4 * cout * cin, self.ld, stream_ptr()), "papc_mlp_bwd_dw_f32")

    def job(self, dw_p, db_p, accumulate):
        """the fields of a ReduceJob that folds dW into ``dw_p`` and, unless ``db_p`` is None, db into ``db_p``"""
        return (self.part.data_ptr(), self.n_chunks, accumulate, self.ld, self.cout * self.cin, self.cout if db_p else 0, dw_p, db_p)

    def fold(self, dw_p, db_p, accumulate):
        """fold now, contiguous dW (papc_reduce_partials2_f32)"""
        check(_lib.load().papc_reduce_partials2_f32(ptr(self.part), self.n_chunks, self.ld, self.cout * self.cin, dw_p, self.cout if db_p else 0,
                                                    db_p, accumulate, stream_ptr()), "papc_reduce_partials2_f32")

    def fold_cols(self, dst_p, dst_ld, accumulate):
        """fold dW now into a column block of a wider matrix: rows of ``dst_ld`` floats from ``dst_p`` (papc_reduce_partials_strided_f32)"""
        check(_lib.load().papc_reduce_partials_strided_f32(ptr(self.part), self.n_chunks, self.ld, self.cout, self.cin, dst_p, dst_ld, accumulate,
                                                           stream_ptr()), "papc_reduce_partials_strided_f32")


# ---- at most 8 jobs per launch ---------------------------------------------------------------------------------------------------------

def launch_batched(struct, jobs, entry, name):
    """``jobs``: tuples in the field order of the ctypes ``struct``; ``entry(array, count, stream)`` takes at most 8 of them per call"""
    st = stream_ptr()
    for k0 in range(0, len(jobs), 8):
        chunk = jobs[k0:k0 + 8]
        check(entry((struct * len(chunk))(*chunk), len(chunk), st), name)
