"""A plain per-row Linear (1x1 conv without norm or activation) on this library's kernels -- the last layer of the part-segmentation
heads, ``conv2`` of /root/reference/PAPC/models/segment/pointnet2/pointnet2.py:49 (logits [B*N, num_parts] from 128 channels).

Forward = papc_mlp_gemm_f32 on plain rows.  The backward reuses the BN-aware row kernels with constants that make their dY the
upstream gradient itself (scale 1, shift huge -> the ReLU mask is always on; mean 0, invstd 1, c1 = c2 = 0): dW and dX are the stack
kernels, the bias gradient is the column sum those kernels' BN-backward reduction produces.  Parameters that opted in to in-place
accumulation (distributed.FlatParams) get their gradients added in place (no AccumulateGrad kernels).

``relu=True`` is relu(rows @ w^T + b), PFNLayer(use_norm=False) of /root/reference/PAPC/models/detect/pointpillars/models/bones/pillars.py:25-27,
:30-32 (Linear with bias + the Empty norm): the forward adds papc_bn_relu_f32 and the backward's shift is 0, so dY = gout * [y > 0].
"""
import ctypes

import torch

from . import _lib
from ._lib import BwdDy, check, ptr, stream_ptr
from .nodeparts import DwPartials, all_or_none, bn_bwd_sums, grad_targets_of, identity_bn


class _LinearRows(torch.autograd.Function):
    """apply(grad targets of (w[, b]) or None, rows [M, Cin], w [Cout, Cin], b [Cout] or None, relu) -> [M, Cout]"""

    @staticmethod
    def forward(ctx, targets, rows, w, b, relu):
        lib = _lib.load()
        st = stream_ptr()
        M, cin = rows.shape
        cout = w.shape[0]
        dev = rows.device
        y = torch.empty(M, cout, device=dev, dtype=torch.float32)
        check(lib.papc_mlp_gemm_f32(0, ptr(rows), cin, None, None, None, ptr(w), ptr(b), M, cin, cout, ptr(y), None, None, st), "papc_mlp_gemm_f32")
        ctx.save_for_backward(rows, w, y)
        ctx.targets, ctx.has_bias, ctx.relu = targets, b is not None, relu
        if not relu:
            return y
        out = torch.empty(M, cout, device=dev, dtype=torch.float32)
        check(lib.papc_bn_relu_f32(ptr(y), ptr(_lib.const_vec(1.0, cout, dev)), ptr(_lib.const_vec(0.0, cout, dev)), M, cout, ptr(out), st),
              "papc_bn_relu_f32")
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        st = stream_ptr()
        rows, w, y = ctx.saved_tensors
        M, cin = rows.shape
        cout = w.shape[0]
        dev = rows.device
        gout = gout.contiguous().float()
        dy = BwdDy()
        dy.dz_mode, dy.dz, dy.gout, dy.argmax, dy.K = 0, gout.data_ptr(), None, None, 1
        identity_bn(dy, y, cout, dev, ctx.relu)
        tg, acc, grads = all_or_none(ctx.targets, [(cout, cin)] + ([(cout,)] if ctx.has_bias else []), dev)
        # dW = dY^T . rows
        part = DwPartials(dy, 0, ptr(rows), cin, None, None, None, M, cin, cout, dev)
        if acc:
            part.fold_cols(ptr(tg[0]), cin, 1)
        else:        # (the partials' bias slot -- the exact 0 of a BN-fed bias -- goes to a scratch vector)
            part.fold(ptr(tg[0]), ptr(torch.empty(cout, device=dev, dtype=torch.float32)), 0)
        # db = column sums of dY: the dbeta of the BN-backward sums under the identity constants (no batch-mean terms: the eval flag)
        if ctx.has_bias:
            bn_bwd_sums(dy, M, cout, torch.empty(2, cout, device=dev, dtype=torch.float32), None, ptr(tg[1]), acc, eval_bn=True)
        dx = None
        if ctx.needs_input_grad[1]:
            wt = torch.empty(cin, cout, device=dev, dtype=torch.float32)
            check(lib.papc_copy2d_f32(ptr(w), cin, ptr(wt), cout, cout, cin, 1, st), "papc_copy2d_f32")
            dx = torch.empty(M, cin, device=dev, dtype=torch.float32)
            check(lib.papc_mlp_bwd_dx_f32(ctypes.byref(dy), ptr(wt), M, cin, cout, ptr(dx), None, None, st), "papc_mlp_bwd_dx_f32")
        return (None, dx) + grads + (None,) * (3 - len(grads))


def linear_rows(rows, weight, bias, relu=False, inplace=True):
    """rows [M, Cin] @ weight[Cout, Cin]^T + bias -> [M, Cout] (``relu``: its ReLU), differentiable, on libpapc_hip.so only.
    ``inplace=False``: the gradients of weight and bias always go back through autograd."""
    if not rows.is_cuda:
        raise _lib.PapcError("linear_rows needs CUDA (ROCm) tensors: there is no CPU fallback")
    w2 = weight.reshape(weight.shape[0], -1)
    tg = None
    if inplace and torch.is_grad_enabled() and w2.data_ptr() == weight.data_ptr():
        tg = grad_targets_of([weight] + ([bias] if bias is not None else []))
    rows = rows if (rows.is_contiguous() and rows.dtype == torch.float32) else rows.contiguous().float()
    return _LinearRows.apply(tg, rows, w2, bias, relu)
