"""The VoxNet classifier's pieces on the library's kernels: the dense 3-D convolution backbone, the head's LeakyReLU + dropout, the occupancy grid.

Reference: PAPC/models/classify/voxnet/voxnet.py:7-25
    backbone = Conv3D(1, 32, 5, 2), BatchNorm(32), LeakyReLU(), Conv3D(32, 32, 3, 1), MaxPool3D(2, 2, 0);  x = reshape(x, (-1, 32 * 6 * 6 * 6))
csrc/voxconv.hip runs both convs as implicit GEMMs on the bf16x3 matrix-pipe bodies: conv1 writes the pre-norm rows y1 [B E1^3, 32] and the
norm's statistics from its epilogue, conv2 applies the norm and the LeakyReLU on load and pools 2x2x2 groups in registers, writing the pooled
values in the source's flatten order and one winner byte per (group, channel).  ``voxconv_backbone`` is ONE autograd node over those launches; it
keeps the input, y1, the norm's constants and the winner bytes -- never the pre-pool tensor or an activation mask.

PAPC_VOXNET=0 (read once, at import) runs the same backbone in torch device ops instead -- each conv a strided-view im2col copy and a matmul
(no convolution-library kernel search), then the norm, leaky_relu and max_pool3d: a second, independent implementation that the tests compare
against, and the baseline of tools/bench_voxnet.py.  Edges outside papc_voxconv_ok take that path too, and so does an eval-mode forward that
records gradients (the kernels' backward is the train-mode norm's).  CPU tensors and non-float32 inputs raise PapcError.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, ptr, stream_ptr
from .nodeparts import all_or_none, grad_targets_of

_VOXNET = os.environ.get("PAPC_VOXNET", "1") != "0"          # A/B switch: 0 = the backbone in torch device ops
BN_MOMENTUM = 0.9            # paddle.nn.BatchNorm's default: the weight of the RUNNING value (models._bn1d, kdnet.BN_MOMENTUM)
SLOPE = 0.01                 # nn.LeakyReLU's default (paddle and torch)
C = 32                       # channels of both convs
EDGE = 32                    # the model's input edge


def edges(E):
    """input edge -> (conv1 edge, conv2 edge, pooled edge)"""
    e1 = (E - 5) // 2 + 1
    return e1, e1 - 2, (e1 - 2) // 2


def kernel_ok(E):
    """whether csrc/voxconv.hip takes this input edge (papc_voxconv_ok)"""
    return _lib.load().papc_voxconv_ok(int(E)) != 0


class _VoxBackbone(torch.autograd.Function):
    """apply(grad targets of (w1, b1, gamma, beta, w2, b2) or None, x [B, 1, E, E, E], w1 [32, 1, 5, 5, 5], b1, gamma, beta, running_mean,
    running_var, w2 [32, 32, 3, 3, 3], b2, eps, training) -> [B, 32 Ep^3].  The input receives no gradient (it is data: an occupancy grid).
    Saved: x, y1, the norm's constants [4, 32] = (mean, 1/sigma, scale, shift), W2 in the dX kernel's K-major order, the winner bytes."""

    @staticmethod
    def forward(ctx, targets, x, w1, b1, gamma, beta, rmean, rvar, w2, b2, eps, training):
        lib, st, dev = _lib.load(), stream_ptr(), x.device
        B, E = x.shape[0], x.shape[2]
        e1, _, ep = edges(E)
        M1, parts = B * e1 ** 3, lib.papc_voxconv_parts(B, E)
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)      # noqa: E731
        y1, part, cst, wk, wt = new(M1, C), new(parts, 2, C), new(4, C), new(C, 27 * C), new(C, 27 * C)
        check(lib.papc_voxconv1_fwd_f32(ptr(x), ptr(w1), ptr(b1), B, E, ptr(y1), ptr(part), st), "papc_voxconv1_fwd_f32")
        if training:
            check(lib.papc_bn_finalize_f32(ptr(part), parts, M1, C, ptr(gamma), ptr(beta), eps, BN_MOMENTUM, *_lib.cst_ptrs(cst), ptr(rmean), ptr(rvar), st),
                  "papc_bn_finalize_f32")
        else:
            check(lib.papc_bn_eval_consts_f32(ptr(rmean), ptr(rvar), ptr(gamma), ptr(beta), eps, C, *_lib.cst_ptrs(cst), st), "papc_bn_eval_consts_f32")
        check(lib.papc_voxconv2_prep_f32(ptr(w2), ptr(wk), ptr(wt), st), "papc_voxconv2_prep_f32")
        out = new(B, C * ep ** 3)
        win = torch.empty(B * ep ** 3, C, device=dev, dtype=torch.uint8)
        check(lib.papc_voxconv2_pool_fwd_f32(ptr(y1), ptr(cst[2]), ptr(cst[3]), ptr(wk), ptr(b2), B, E, ptr(out), ptr(win), st), "papc_voxconv2_pool_fwd_f32")
        ctx.save_for_backward(x, y1, cst, wt, win)
        ctx.dims, ctx.targets, ctx.parts = (B, E), targets, parts
        return out

    @staticmethod
    def backward(ctx, gout):
        x, y1, cst, wt, win = ctx.saved_tensors
        B, E = ctx.dims
        lib, st, dev = _lib.load(), stream_ptr(), x.device
        e1, _, ep = edges(E)
        M1 = B * e1 ** 3
        gout = gout.contiguous().float()
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)      # noqa: E731
        (dw1, db1, dgamma, dbeta, dw2, db2), acc, grads = all_or_none(ctx.targets, [(C, 1, 5, 5, 5), (C,), (C,), (C,), (C, C, 3, 3, 3), (C,)], dev)
        gp, dz, red, c12 = new(B * ep ** 3, C), new(M1, C), new(ctx.parts, 2, C), new(2, C)
        mean, invstd, scale, shift = _lib.cst_ptrs(cst)
        check(lib.papc_voxconv2_bwd_dx_f32(ptr(gout), ptr(win), ptr(wt), ptr(y1), mean, invstd, scale, shift, B, E, ptr(gp), ptr(dz), ptr(red), st),
              "papc_voxconv2_bwd_dx_f32")
        check(lib.papc_bn_bwd_finalize_f32(ptr(red), ctx.parts, M1, C, ptr(dgamma), ptr(dbeta), ptr(c12[0]), ptr(c12[1]), acc, st), "papc_bn_bwd_finalize_f32")
        nb = lib.papc_voxconv2_bwd_dw_workspace(B, E)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        check(lib.papc_voxconv2_bwd_dw_f32(ptr(gp), ptr(win), ptr(y1), scale, shift, B, E, ptr(dw2), ptr(db2), acc, ptr(ws), nb, st), "papc_voxconv2_bwd_dw_f32")
        nb = lib.papc_voxconv1_bwd_dw_workspace(B, E)
        ws = torch.empty(nb, device=dev, dtype=torch.uint8)
        check(lib.papc_voxconv1_bwd_dw_f32(ptr(dz), ptr(y1), mean, invstd, scale, ptr(c12[0]), ptr(c12[1]), ptr(x), B, E, ptr(dw1), ptr(db1), acc, ptr(ws), nb,
                                           st), "papc_voxconv1_bwd_dw_f32")
        g = grads
        return (None, None, g[0], g[1], g[2], g[3], None, None, g[4], g[5], None, None)


def _im2col(v, k, stride):
    """v [B, D, H, W, C] -> patches [B, D', H', W', C, k, k, k] as a strided view (no copy)"""
    return v.unfold(1, k, stride).unfold(2, k, stride).unfold(3, k, stride)


def _backbone_torch(x, conv1, bn, conv2, training):
    """voxnet.py:8-12 in torch device ops: each conv the im2col copy of a strided view and a matmul; the norm with the convention of
    models._bn1d (the biased batch variance goes into the running estimate, as paddle.nn.BatchNorm does) -> [B, 32 Ep^3]"""
    B, E = x.shape[0], x.shape[2]
    e1, e2, _ = edges(E)
    rows = _im2col(x.reshape(B, E, E, E, 1), 5, 2).reshape(B * e1 ** 3, 125)                      # the copy; K order (tz, ty, tx)
    y = torch.matmul(rows, conv1.weight.view(C, 125).t()) + (conv1.bias if conv1.bias is not None else 0.0)
    if training:
        mean = y.mean(0)
        var = y.var(0, unbiased=False)
        with torch.no_grad():
            bn.running_mean.mul_(BN_MOMENTUM).add_(mean.detach(), alpha=1.0 - BN_MOMENTUM)
            bn.running_var.mul_(BN_MOMENTUM).add_(var.detach(), alpha=1.0 - BN_MOMENTUM)
    else:
        mean, var = bn.running_mean, bn.running_var
    a = F.leaky_relu((y - mean) / torch.sqrt(var + bn.eps) * bn.weight + bn.bias, SLOPE)
    rows = _im2col(a.view(B, e1, e1, e1, C), 3, 1).reshape(B * e2 ** 3, C * 27)                    # K order (ci, tz, ty, tx): the weight's own
    y = torch.matmul(rows, conv2.weight.view(C, C * 27).t()) + (conv2.bias if conv2.bias is not None else 0.0)
    y = F.max_pool3d(y.view(B, e2, e2, e2, C).permute(0, 4, 1, 2, 3), 2, 2)
    return y.reshape(B, -1)


def voxconv_backbone(x, conv1, bn, conv2, training):
    """The VoxNet backbone, flattened.  x [B, 1, E, E, E] float32 on the device (the model has E = 32), conv1 = nn.Conv3d(1, 32, 5, 2),
    bn = nn.BatchNorm3d(32) (its running statistics are updated in train mode and read in eval mode), conv2 = nn.Conv3d(32, 32, 3, 1)
    -> [B, 32 Ep^3] in the source's flatten order.  Gradients reach conv1, bn and conv2 -- conv1.bias receives exact zeros in train mode -- and
    NOT x.  One autograd node on csrc/voxconv.hip; PAPC_VOXNET=0, edges outside papc_voxconv_ok and an eval-mode forward under autograd run
    torch device ops."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.PapcError("voxconv_backbone needs CUDA (ROCm) tensors: there is no CPU fallback")
    if x.dtype != torch.float32:
        raise _lib.PapcError("voxconv_backbone takes a float32 grid, got %s" % x.dtype)
    if x.dim() != 5 or x.shape[1] != 1 or not (x.shape[2] == x.shape[3] == x.shape[4]) or x.shape[2] < 9:
        raise _lib.PapcError("voxconv_backbone: a grid [B, 1, E, E, E] (E >= 9) expected, got %s" % (tuple(x.shape),))
    if tuple(conv1.weight.shape) != (C, 1, 5, 5, 5) or tuple(conv2.weight.shape) != (C, C, 3, 3, 3) or bn.num_features != C or bn.weight is None \
            or bn.running_mean is None or conv1.stride != (2, 2, 2) or conv2.stride != (1, 1, 1):
        raise _lib.PapcError("voxconv_backbone: Conv3d(1, 32, 5, 2), an affine BatchNorm3d(32) with running statistics and Conv3d(32, 32, 3, 1) expected")
    E = int(x.shape[2])
    grad = torch.is_grad_enabled() and any(p.requires_grad for p in (conv1.weight, bn.weight, conv2.weight))
    if not (_VOXNET and kernel_ok(E) and conv1.bias is not None and conv2.bias is not None and (training or not grad)):
        return _backbone_torch(x, conv1, bn, conv2, training)
    params = [conv1.weight, conv1.bias, bn.weight, bn.bias, conv2.weight, conv2.bias]
    tg = grad_targets_of(params) if torch.is_grad_enabled() else None
    return _VoxBackbone.apply(tg, x.contiguous(), conv1.weight, conv1.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, conv2.weight, conv2.bias,
                              float(bn.eps), bool(training))


# ---- the head's LeakyReLU + Dropout ------------------------------------------------------------------------------------------------------

class _LeakyDropout(torch.autograd.Function):
    """apply(spec (head.HeadSpec: the device rng state, the mask export), x [B, C], p, training) -> dropout(leaky_relu(x)), upscale in train"""

    @staticmethod
    def forward(ctx, spec, x, p, training):
        lib, dev = _lib.load(), x.device
        x = x.contiguous()
        drop = training and p > 0.0
        out = torch.empty_like(x)
        keep = torch.empty(x.shape, device=dev, dtype=torch.uint8) if drop else None
        rng = spec.state(dev) if drop else None
        check(lib.papc_leaky_dropout_fwd_f32(ptr(x), x.numel(), SLOPE, p if drop else 0.0, ptr(rng), 1, 1, ptr(out), ptr(keep), stream_ptr()),
              "papc_leaky_dropout_fwd_f32")
        if spec.export_masks:
            spec.masks = (keep,)
        ctx.save_for_backward(x, keep)
        ctx.p = p if drop else 0.0
        return out

    @staticmethod
    def backward(ctx, gout):
        x, keep = ctx.saved_tensors
        gout = gout.contiguous().float()
        dx = torch.empty_like(x)
        check(_lib.load().papc_leaky_dropout_bwd_f32(ptr(gout), ptr(x), ptr(keep), x.numel(), SLOPE, ctx.p, ptr(dx), stream_ptr()), "papc_leaky_dropout_bwd_f32")
        return None, dx, None, None


def leaky_dropout(spec, x, p, training):
    """dropout(leaky_relu(x [B, C]), p) as one launch each way (voxnet.py:16-17); the mask is the head's counter hash of ``spec``'s device
    rng state, so a replayed graph draws a fresh one.  ``training=False``: no dropout."""
    if not x.is_cuda or x.dtype != torch.float32:
        raise _lib.PapcError("leaky_dropout needs float32 CUDA (ROCm) tensors: there is no CPU fallback")
    return _LeakyDropout.apply(spec, x, float(p), bool(training))


# ---- the occupancy grid --------------------------------------------------------------------------------------------------------------------

def occupancy_grid_np(points, edge=EDGE):
    """The host twin: points [B, N, 3] (float32) in [-1, 1] -> [B, 1, edge, edge, edge] float32 with 1.0 at (int(x h + h), int(y h + h),
    int(z h + h)), h = (edge - 1) / 2 (PAPC/datasets/tools/build_VoxData.py:58-60 has edge = 32, h = 15.5).  The index is evaluated in float64
    from the float32 coordinate.  A coordinate outside [-1, 1] raises (the source's index would wrap around or overflow the array)."""
    pts = np.asarray(points, dtype=np.float32)
    if pts.ndim != 3 or pts.shape[2] != 3:
        raise _lib.PapcError("occupancy_grid: points [B, N, 3] expected, got %s" % (pts.shape,))
    if not bool(np.all((pts >= -1.0) & (pts <= 1.0))):
        raise _lib.PapcError("occupancy_grid: %d coordinates outside [-1, 1]" % int(np.sum(~((pts >= -1.0) & (pts <= 1.0)))))
    h = (edge - 1) / 2.0
    idx = (pts.astype(np.float64) * h + h).astype(np.int64)                                      # truncation, as int() does
    grid = np.zeros((pts.shape[0], 1, edge, edge, edge), np.float32)
    b = np.repeat(np.arange(pts.shape[0]), pts.shape[1])
    grid[b, 0, idx[..., 0].reshape(-1), idx[..., 1].reshape(-1), idx[..., 2].reshape(-1)] = 1.0
    return grid


def occupancy_grid(points, edge=EDGE):
    """points [B, N, 3] float32 on the device -> the occupancy grid [B, 1, edge, edge, edge] of occupancy_grid_np, bit for bit.  The device
    clamps a coordinate outside [-1, 1] and counts it; the count is read back here (one synchronisation) and raises PapcError."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise _lib.PapcError("occupancy_grid needs a CUDA (ROCm) tensor: there is no CPU fallback (occupancy_grid_np is the host twin)")
    if points.dtype != torch.float32 or points.dim() != 3 or points.shape[2] != 3:
        raise _lib.PapcError("occupancy_grid: float32 points [B, N, 3] expected, got %s %s" % (points.dtype, tuple(points.shape)))
    points = points.contiguous()
    B, N = points.shape[0], points.shape[1]
    grid = torch.empty(B, 1, edge, edge, edge, device=points.device, dtype=torch.float32)
    err = torch.empty(1, device=points.device, dtype=torch.int32)
    check(_lib.load().papc_occupancy_grid_f32(ptr(points), B, N, int(edge), ptr(grid), ptr(err), stream_ptr()), "papc_occupancy_grid_f32")
    bad = int(err.item())
    if bad:
        raise _lib.PapcError("occupancy_grid: %d points with a coordinate outside [-1, 1]" % bad)
    return grid
