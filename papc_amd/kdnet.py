"""One level of the KD-Net classifier on the library's kernels: relu(conv), the kd-tree select, the max over adjacent point pairs.

Reference: PAPC/models/classify/kdnet/kdnet.py:21-30
    x = relu(conv(x));  x = reshape(x, (-1, F, 3, dim));  x = reshape(x, (-1, F, 3 * dim))
    x = index_select(x, axis=2, index=select + 3 * arange(dim));  x = max(reshape(x, (-1, F, dim / 2, 2)), axis=-1)
csrc/kdconv.hip computes only the selected third of the conv and pools the pairs in registers; the autograd node keeps the level's input
rows, its output and one winner byte per output element, never the [B * dim, 3F] activations.  Rows are point-major ([B * dim, C]).

PAPC_KDCONV=0 (read once, at import) runs the source's op sequence in torch device ops instead -- the 1x1 conv (written as the matmul it
is: no convolution-library kernel search), the two reshapes, one index_select per cloud, the reshape and the max: a second, independent
implementation that the tests compare against, and the baseline of tools/bench_kdnet.py.  Shapes outside papc_kdconv_ok take that path as
well.  CPU tensors and non-float32 rows raise PapcError.

kdconv_bn is the down level of the KDUNet part segmenter (PAPC/models/segment/kdunet/kdunet.py:51-61): the same level with a BatchNorm over all
3F channels between the conv and the ReLU.  csrc/kdbn.hip takes the norm's statistics, and the dense part of its backward, from the mean and
the Cin x Cin second moment of the level's input rows, so it too computes only the selected third of the conv.  The same switch
and the same rules apply.

Split dims: ten vectors of lengths 1024, 512, ... 2 per cloud, values in 0..2.  On the device they are ONE packed int32 tensor, [2046]
(shared by every cloud, the source's one-cloud form) or [B, 2046]; a level reads its slice in place.
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .nodeparts import all_or_none, grad_targets_of

_KDCONV = os.environ.get("PAPC_KDCONV", "1") != "0"          # A/B switch: 0 = the source's op sequence in torch device ops
DIMS = (1024, 512, 256, 128, 64, 32, 16, 8, 4, 2)            # points per cloud entering level 1 .. 10 (kdnet.py:35-44)
PACKED = sum(DIMS)                                            # 2046
OFFSETS = tuple(int(v) for v in np.cumsum((0,) + DIMS[:-1]))


def kernel_ok(dim, cin, f):
    """whether csrc/kdconv.hip takes this level (papc_kdconv_ok)"""
    return _lib.load().papc_kdconv_ok(int(dim), int(cin), int(f)) != 0


class _KDConv(torch.autograd.Function):
    """apply(grad targets, rows [B*dim, Cin], sel int32 [dim] or [B, dim] (a view), w [3F, Cin], bias [3F] or None, B, dim) -> [B*dim/2, F]"""

    @staticmethod
    def forward(ctx, targets, rows, sel, w, b, B, dim):
        lib = _lib.load()
        M, cin = rows.shape
        f = w.shape[0] // 3
        ss = 0 if sel.dim() == 1 else sel.stride(0)
        out = torch.empty(M // 2, f, device=rows.device, dtype=torch.float32)
        win = torch.empty(M // 2, f, device=rows.device, dtype=torch.uint8)
        check(lib.papc_kdconv_fwd_f32(ptr(rows), rows.stride(0), ptr(sel), ss, ptr(w), ptr(b), B, dim, cin, f, ptr(out), ptr(win), stream_ptr()),
              "papc_kdconv_fwd_f32")
        ctx.save_for_backward(rows, sel, w, out, win)
        ctx.dims = (B, dim, cin, f, ss)
        ctx.targets = targets
        ctx.has_bias = b is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        rows, sel, w, out, win = ctx.saved_tensors
        B, dim, cin, f, ss = ctx.dims
        lib = _lib.load()
        dev = rows.device
        gout = gout.contiguous().float()
        tg, acc, grads = all_or_none(ctx.targets, [(3 * f, cin)] + ([(3 * f,)] if ctx.has_bias else []), dev)
        dw, db = tg[0], (tg[1] if ctx.has_bias else None)
        dx = torch.empty(B * dim, cin, device=dev, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        nbytes = lib.papc_kdconv_bwd_workspace(B, dim, cin, f)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        check(lib.papc_kdconv_bwd_f32(ptr(gout), ptr(out), ptr(win), ptr(rows), rows.stride(0), ptr(sel), ss, ptr(w), B, dim, cin, f, ptr(dx), cin,
                                      ptr(dw), ptr(db), acc, ptr(ws), nbytes, stream_ptr()), "papc_kdconv_bwd_f32")
        return (None, dx, None) + grads + (None,) * (4 - len(grads))


def _kdconv_torch(rows, sel, conv, B, dim):
    """kdnet.py:21-30 op by op, on [B, C, dim] tensors"""
    cin = rows.shape[1]
    f = conv.out_channels // 3
    x = rows.view(B, dim, cin).transpose(1, 2)                                                    # [B, Cin, dim]
    x = torch.relu(torch.matmul(conv.weight.view(3 * f, cin), x) + (conv.bias.view(1, -1, 1) if conv.bias is not None else 0.0))   # :22
    return _select_max_torch(x, sel, B, dim, f)


def _select_max_torch(x, sel, B, dim, f):
    """kdnet.py:23-28 / kdunet.py:54-59 op by op: x [B, 3F, dim] -> rows [B * dim / 2, F]"""
    x = x.reshape(-1, f, 3, dim)                                                                   # :23
    x = x.reshape(-1, f, 3 * dim)                                                                  # :24
    ar = torch.arange(0, dim, device=x.device) * 3
    if sel.dim() == 1:
        x = torch.index_select(x, 2, sel.long() + ar)                                              # :25-26
    else:                                                                                          # one split vector per cloud: the source's call per cloud
        x = torch.stack([torch.index_select(x[b], 1, sel[b].long() + ar) for b in range(B)])
    x = x.reshape(-1, f, dim // 2, 2)                                                              # :27
    x = torch.max(x, dim=-1)[0]                                                                    # :28
    return x.transpose(1, 2).reshape(B * (dim // 2), f)


def _check_level(who, rows, sel, conv, B, dim):
    """the argument rules both level nodes share -> (B, dim, Cin, 3F)"""
    if not rows.is_cuda or not sel.is_cuda:
        raise _lib.PapcError("%s needs CUDA (ROCm) tensors: there is no CPU fallback" % who)
    if rows.dtype != torch.float32:
        raise _lib.PapcError("%s takes float32 rows, got %s" % (who, rows.dtype))
    if sel.dtype != torch.int32:
        raise _lib.PapcError("%s takes int32 split dims, got %s" % (who, sel.dtype))
    B, dim = int(B), int(dim)
    cin, cout = conv.in_channels, conv.out_channels
    if rows.dim() != 2 or rows.shape[0] != B * dim or rows.shape[1] != cin or cout % 3 or sel.shape[-1] != dim or (sel.dim() == 2 and sel.shape[0] != B) \
            or sel.dim() > 2 or sel.stride(-1) != 1:
        raise _lib.PapcError("%s: rows [B*dim, Cin] = [%d, %d], split dims [%d] or [%d, %d] and a conv to 3F channels expected, got %s, %s and %d"
                             % (who, B * dim, cin, dim, B, dim, tuple(rows.shape), tuple(sel.shape), cout))
    return B, dim, cin, cout


def _kernel_rows(rows, cin):
    """rows as the MFMA kernels load them: unit column stride, 16-byte aligned rows (Cin = 3 reads scalars)"""
    if not (rows.stride(1) == 1 and (cin == 3 or (rows.stride(0) % 4 == 0 and rows.data_ptr() % 16 == 0))):
        rows = rows.contiguous()
    return rows


def kdconv(rows, sel, conv, B, dim):
    """One KD-Net level.  rows [B*dim, Cin] float32 point-major, sel int32 split dims [dim] (shared by every cloud) or [B, dim] (may be a
    view of the packed tensor), conv = nn.Conv1d(Cin, 3F, 1) (its weight read in place) -> [B*dim/2, F].  Gradients reach rows and conv."""
    B, dim, cin, cout = _check_level("kdconv", rows, sel, conv, B, dim)
    if not (_KDCONV and kernel_ok(dim, cin, cout // 3)):
        return _kdconv_torch(rows, sel, conv, B, dim)
    rows = _kernel_rows(rows, cin)
    tg = grad_targets_of([conv.weight] + ([conv.bias] if conv.bias is not None else [])) if torch.is_grad_enabled() else None
    return _KDConv.apply(tg, rows, sel, conv.weight.view(cout, cin), conv.bias, B, dim)


# ---- the KDUNet down level: conv + BatchNorm + ReLU + select + pair max (csrc/kdbn.hip) ---------------------------------------------------

BN_MOMENTUM = 0.9            # paddle.nn.BatchNorm's default: the weight of the RUNNING value (models._bn1d, StackSpec)


def bn_kernel_ok(dim, cin, f):
    """whether csrc/kdbn.hip takes this level (papc_kdbn_ok)"""
    return _lib.load().papc_kdbn_ok(int(dim), int(cin), int(f)) != 0


class _KDConvBN(torch.autograd.Function):
    """apply(grad targets of (w, bias, gamma, beta) or None, rows [B*dim, Cin], sel, w [3F, Cin], bias [3F] or None, gamma, beta [3F],
    running_mean, running_var [3F], B, dim, eps, training) -> [B*dim/2, F].  Saved: rows, sel, w, gamma, out, the winner bytes, the winners'
    normalised values, the rows' mean [Cin], T = W C [3F, Cin] and stats [4, 3F] = (w . mean | 1/sigma | mu | var)."""

    @staticmethod
    def forward(ctx, targets, rows, sel, w, b, gamma, beta, rmean, rvar, B, dim, eps, training):
        lib = _lib.load()
        dev = rows.device
        M, cin = rows.shape
        f = w.shape[0] // 3
        ss = 0 if sel.dim() == 1 else sel.stride(0)
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)      # noqa: E731
        out, zhat, stats = new(M // 2, f), new(M // 2, f), new(4, 3 * f)
        win = torch.empty(M // 2, f, device=dev, dtype=torch.uint8)
        mean = tmat = ws = None
        nbytes = 0
        if training:
            mean, tmat = new(cin), new(3 * f, cin)
            nbytes = lib.papc_kdbn_fwd_workspace(B, dim, cin, f)
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        check(lib.papc_kdbn_fwd_f32(ptr(rows), rows.stride(0), ptr(sel), ss, ptr(w), ptr(b), ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), B, dim, cin, f,
                                    eps, BN_MOMENTUM, 1 if training else 0, ptr(out), ptr(win), ptr(zhat), ptr(mean), ptr(tmat), ptr(stats), ptr(ws),
                                    nbytes, stream_ptr()), "papc_kdbn_fwd_f32")
        ctx.save_for_backward(rows, sel, w, gamma, out, win, zhat, mean, tmat, stats)
        ctx.dims = (B, dim, cin, f, ss, training)
        ctx.targets = targets
        ctx.has_bias = b is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        rows, sel, w, gamma, out, win, zhat, mean, tmat, stats = ctx.saved_tensors
        B, dim, cin, f, ss, training = ctx.dims
        lib = _lib.load()
        dev = rows.device
        gout = gout.contiguous().float()
        shapes = [(3 * f, cin)] + ([(3 * f,)] if ctx.has_bias else []) + [(3 * f,), (3 * f,)]
        tg, acc, grads = all_or_none(ctx.targets, shapes, dev)
        dw, db = tg[0], (tg[1] if ctx.has_bias else None)
        dgamma, dbeta = tg[-2], tg[-1]
        dx = torch.empty(B * dim, cin, device=dev, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        nbytes = lib.papc_kdbn_bwd_workspace(B, dim, cin, f)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        check(lib.papc_kdbn_bwd_f32(ptr(gout), ptr(out), ptr(win), ptr(zhat), ptr(rows), rows.stride(0), ptr(sel), ss, ptr(w), ptr(gamma), ptr(mean),
                                    ptr(tmat), ptr(stats), B, dim, cin, f, 1 if training else 0, ptr(dx), cin, ptr(dw), ptr(db), ptr(dgamma), ptr(dbeta),
                                    acc, ptr(ws), nbytes, stream_ptr()), "papc_kdbn_bwd_f32")
        gw = grads[0]
        gb = grads[1] if ctx.has_bias else None
        return (None, dx, None, gw, gb, grads[-2], grads[-1]) + (None,) * 6


def _kdconv_bn_torch(rows, sel, conv, bn, B, dim, training):
    """kdunet.py:51-61 op by op, on [B, C, dim] tensors; the norm with the convention of models._bn1d (the biased batch variance goes into
    the running estimate, as paddle.nn.BatchNorm does)"""
    cin = rows.shape[1]
    f = conv.out_channels // 3
    x = rows.view(B, dim, cin).transpose(1, 2)                                                    # [B, Cin, dim]
    y = torch.matmul(conv.weight.view(3 * f, cin), x) + (conv.bias.view(1, -1, 1) if conv.bias is not None else 0.0)    # :36 (ConvBNReLU)
    if training:
        mean = y.mean((0, 2))
        var = y.var((0, 2), unbiased=False)
        with torch.no_grad():
            bn.running_mean.mul_(BN_MOMENTUM).add_(mean.detach(), alpha=1.0 - BN_MOMENTUM)
            bn.running_var.mul_(BN_MOMENTUM).add_(var.detach(), alpha=1.0 - BN_MOMENTUM)
    else:
        mean, var = bn.running_mean, bn.running_var
    y = (y - mean.view(1, -1, 1)) / torch.sqrt(var.view(1, -1, 1) + bn.eps) * bn.weight.view(1, -1, 1) + bn.bias.view(1, -1, 1)   # :37
    return _select_max_torch(torch.relu(y), sel, B, dim, f)                                        # :38, :54-59


def kdconv_bn(rows, sel, conv, bn, B, dim, training):
    """One KDUNet down level.  rows [B*dim, Cin] float32 point-major, sel as for kdconv, conv = nn.Conv1d(Cin, 3F, 1), bn = nn.BatchNorm1d(3F)
    (its running statistics are updated in train mode and read in eval mode) -> [B*dim/2, F].  Gradients reach rows, conv and bn; the conv
    bias receives exact zeros in train mode.  One autograd node on csrc/kdbn.hip; PAPC_KDCONV=0 and shapes outside papc_kdbn_ok run the
    source's op sequence in torch device ops."""
    B, dim, cin, cout = _check_level("kdconv_bn", rows, sel, conv, B, dim)
    if bn.num_features != cout or bn.weight is None or bn.running_mean is None:
        raise _lib.PapcError("kdconv_bn: an affine BatchNorm1d(%d) with running statistics expected" % cout)
    if not (_KDCONV and bn_kernel_ok(dim, cin, cout // 3)):
        return _kdconv_bn_torch(rows, sel, conv, bn, B, dim, training)
    rows = _kernel_rows(rows, cin)
    params = [conv.weight] + ([conv.bias] if conv.bias is not None else []) + [bn.weight, bn.bias]
    tg = grad_targets_of(params) if torch.is_grad_enabled() else None
    return _KDConvBN.apply(tg, rows, sel, conv.weight.view(cout, cin), conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, B, dim,
                           float(bn.eps), bool(training))


def pack_split_dims(split_dims, B, device):
    """The source's split dims -> one int32 device tensor [2046] (one vector per level, shared by every cloud) or [B, 2046].

    Takes the packed form itself (tensor or numpy, [2046] or [B, 2046]) or the source's list of ten arrays, each [dim_l] or [B, dim_l] with
    dim_l = 1024, 512, ... 2 (kdnet.py:35-44, datasets/kdloader.py:38-41).  A list is packed on the host and copied once.  Numpy values
    outside 0..2 raise PapcError (device tensors are not read back: the kernel clamps)."""
    def bad(msg):
        return _lib.PapcError("KDNet split dims: " + msg)

    if isinstance(split_dims, torch.Tensor):
        t = split_dims
        if not t.is_cuda:
            raise bad("a tensor must be on the CUDA (ROCm) device (numpy arrays are copied there)")
    else:
        if isinstance(split_dims, np.ndarray) and split_dims.dtype != object and split_dims.shape[-1:] == (PACKED,):
            a = split_dims
        else:
            levels = list(split_dims)
            if len(levels) != len(DIMS):
                raise bad("%d levels given, %d expected" % (len(levels), len(DIMS)))
            if all(isinstance(v, torch.Tensor) and v.is_cuda for v in levels):
                per_cloud = any(v.dim() == 2 for v in levels)
                t = torch.cat([(v if v.dim() == 2 or not per_cloud else v.view(1, -1).expand(B, -1)).to(torch.int32) for v in levels], -1)
                return pack_split_dims(t, B, device)
            levels = [np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v) for v in levels]
            for v, d in zip(levels, DIMS):
                if v.ndim not in (1, 2) or v.shape[-1] != d or (v.ndim == 2 and v.shape[0] != B):
                    raise bad("a level of shape %s where [%d] or [%d, %d] is expected" % (v.shape, d, B, d))
            per_cloud = any(v.ndim == 2 for v in levels)
            a = np.empty((B, PACKED) if per_cloud else (PACKED,), np.int32)
            for v, d, o in zip(levels, DIMS, OFFSETS):
                a[..., o:o + d] = v
        if a.size and (a.min() < 0 or a.max() > 2):
            raise bad("values must be 0, 1 or 2 (found %d .. %d)" % (int(a.min()), int(a.max())))
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
    if t.dim() not in (1, 2) or t.shape[-1] != PACKED or (t.dim() == 2 and t.shape[0] != B):
        raise bad("packed shape %s where [%d] or [%d, %d] is expected" % (tuple(t.shape), PACKED, B, PACKED))
    if t.dtype != torch.int32 or t.stride(-1) != 1:
        t = t.to(torch.int32).contiguous()
    return t


def level_split_dims(packed, level):
    """the split dims of level 0..9 as a view of the packed tensor"""
    o, d = OFFSETS[level], DIMS[level]
    return packed[..., o:o + d]
