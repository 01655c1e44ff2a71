"""The per-cloud transform of the T-Net PointNet and its T-Net FC blocks on the library's kernels.

Reference: /root/reference/PAPC/models/classify/pointnet/pointnet_Conv1D.py
    :85-88   x = transpose(matmul(transpose(x), T_in))      T_in  [B, 3, 3]    (input transform of the planar [B, 3, N] points)
    :96-99   x = transpose(matmul(transpose(x), T_feat))    T_feat [B, 64, 64] (feature transform of mlp_1's output)
    :19-28, :50-56   input_fc / feature_fc: Linear-ReLU-Linear-ReLU-Linear (no dropout) -> the T-Net's matrix
The transform is csrc/cloud_transform.hip (one launch forward; two backward: dX and the per-chunk partial dT in one pass over dY, then a
fixed-order fold -- bit-reproducible).  The FC blocks are the PointNet-Basic head kernels (head._HeadPlain, p = 0); a last layer whose width
is no multiple of 4 (input_fc's 9) runs padded to the next multiple of 4 inside the node.  CPU tensors raise PapcError: there is no CPU path.
"""
import torch

from . import _lib
from . import head as _head
from ._lib import check, ptr, stream_ptr
from .copyops import _launch as _copy_launch


class _CloudTransform(torch.autograd.Function):
    """apply(x, T, B, N, C, xs, dxs): y [B, N, C] with y[b, n] = x[b, n] . T[b] (T [B, C, C], rows of each matrix contiguous); x element (b, n, i) at x.data_ptr() + xs . (b, n, i)
    (in elements), the gradient for x in a fresh tensor of x's shape whose element strides are ``dxs``."""

    @staticmethod
    def forward(ctx, x, T, B, N, C, xs, dxs):
        if T.stride(2) != 1 or T.stride(1) != C:      # (each matrix row-major; the clouds may sit at any pitch, e.g. a padded T-Net output)
            T = T.contiguous()
        y = torch.empty(B, N, C, device=x.device, dtype=torch.float32)
        check(_lib.load().papc_cloud_transform_f32(ptr(x), xs[0], xs[1], xs[2], ptr(T), T.stride(0), B, N, C, ptr(y), stream_ptr()),
              "papc_cloud_transform_f32")
        ctx.dims, ctx.xs, ctx.dxs = (B, N, C), xs, dxs
        ctx.save_for_backward(x, T)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, T = ctx.saved_tensors
        B, N, C = ctx.dims
        xs, dxs = ctx.xs, ctx.dxs
        lib = _lib.load()
        gy = gy.contiguous().float()
        dev = gy.device
        dx = torch.empty(x.shape, device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        dT = torch.empty(B, C, C, device=dev, dtype=torch.float32)
        nbytes = lib.papc_cloud_transform_bwd_workspace(B, N, C)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        check(lib.papc_cloud_transform_bwd_f32(ptr(x), xs[0], xs[1], xs[2], ptr(T), T.stride(0), ptr(gy), B, N, C, ptr(dx), dxs[0], dxs[1], dxs[2], 0,
                                               ptr(dT), ptr(ws), nbytes, stream_ptr()), "papc_cloud_transform_bwd_f32")
        return dx, dT, None, None, None, None, None


def _check_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise _lib.PapcError("the per-cloud transform needs CUDA (ROCm) tensors: there is no CPU fallback")
        if t.dtype != torch.float32:
            raise _lib.PapcError("the per-cloud transform takes float32 tensors, got %s" % t.dtype)


def transform_points(x, T):
    """x [B, C, N] planar (any strides; the model's input, C = 3), T [B, C, C] -> [B, N, C] contiguous = x^T . T per cloud
    (pointnet_Conv1D.py:85-87 without the transposes: the result is the [B*N, C] row operand of the next stack)."""
    _check_cuda(x, T)
    B, C, N = x.shape
    if tuple(T.shape) != (B, C, C):
        raise _lib.PapcError("transform_points: T must be [B, C, C] = [%d, %d, %d], got %s" % (B, C, C, tuple(T.shape)))
    s = x.stride()
    return _CloudTransform.apply(x, T, B, N, C, (s[0], s[2], s[1]), (C * N, 1, N))


def transform_rows(x, T, N):
    """x [B*N, C] point-major rows (any row stride, unit column stride), T [B, C, C] -> [B*N, C] contiguous: every cloud's rows times its
    own matrix (pointnet_Conv1D.py:96-99 on mlp_1's row output)."""
    _check_cuda(x, T)
    B, C = T.shape[0], x.shape[1]
    if tuple(T.shape) != (B, C, C) or x.shape[0] != B * N:
        raise _lib.PapcError("transform_rows: x [B*N, C] = [%d, %d] and T [B, C, C] = [%d, %d, %d] expected, got %s and %s"
                             % (B * N, C, B, C, C, tuple(x.shape), tuple(T.shape)))
    s = x.stride()
    return _CloudTransform.apply(x, T, B, N, C, (N * s[0], s[0], s[1]), (N * C, C, 1)).view(B * N, C)


class _HeadPlainPadded(torch.autograd.Function):
    """_HeadPlain (Linear-ReLU-Linear-ReLU-[Dropout]-Linear) whose last layer has Cout % 4 != 0: the head kernels' dX of layer 2 reads the
    logits' gradient rows and W3 in float4 pieces along Cout (head.hip: mfma_g_times_w), so that layer runs as ceil4(Cout) rows with zero
    weight and bias rows appended.  The output is the first Cout columns; the gradient goes back padded with zero columns, and the padded
    rows of dW3 / db3 (zero) are dropped.  One strided-copy launch pads W3 and b3, one pads the gradient."""

    @staticmethod
    def forward(ctx, spec, p, x0, w1, b1, w2, b2, w3, b3):
        c3, cin = w3.shape
        cp = (c3 + 3) // 4 * 4
        dev = x0.device
        z = _lib.const_zeros((1,), dev)
        w3p = torch.empty(cp, cin, device=dev, dtype=torch.float32)
        b3p = torch.empty(cp, device=dev, dtype=torch.float32)
        w3c, b3c = w3.contiguous(), b3.contiguous()
        _copy_launch([(w3c, 0, (0, cin, 1), w3p, 0, (0, cin, 1), 1, c3, cin),
                      (z, 0, (0, 0, 0), w3p, c3 * cin, (0, cin, 1), 1, cp - c3, cin),
                      (b3c, 0, (0, 0, 1), b3p, 0, (0, 0, 1), 1, 1, c3),
                      (z, 0, (0, 0, 0), b3p, c3, (0, 0, 1), 1, 1, cp - c3)])
        logits = _head._HeadPlain.forward(ctx, spec, p, x0, w1, b1, w2, b2, w3p, b3p)
        ctx.c3 = c3
        return logits[:, :c3]

    @staticmethod
    def backward(ctx, g):
        c3 = ctx.c3
        B = g.shape[0]
        w3p = ctx.saved_tensors[3]
        cp = w3p.shape[0]
        z = _lib.const_zeros((1,), g.device)
        gp = torch.empty(B, cp, device=g.device, dtype=torch.float32)
        g = g.float()
        _copy_launch([(g, 0, (0, g.stride(0), g.stride(1)), gp, 0, (0, cp, 1), 1, B, c3),
                      (z, 0, (0, 0, 0), gp, c3, (0, cp, 1), 1, B, cp - c3)])
        grads = _head._HeadPlain.backward(ctx, gp)
        dw3, db3 = grads[-2], grads[-1]
        return grads[:-2] + (dw3[:c3], db3[:c3])


_NO_DROPOUT = torch.nn.Dropout(0.0)


def tnet_fc(spec, x, fc):
    """fc = nn.Sequential(Linear, ReLU, Linear, ReLU, Linear) of a T-Net (pointnet_Conv1D.py:19-28, :50-56) on the head kernels, rows
    [B, Cin] -> [B, Cout].  No dropout (p = 0).  ``spec`` = the block's head.HeadSpec."""
    if not x.is_cuda:
        raise _lib.PapcError("the T-Net FC block needs CUDA (ROCm) tensors: there is no CPU fallback")
    fc1, fc2, fc3 = fc[0], fc[2], fc[4]
    if not (x.dtype == torch.float32 and x.dim() == 2 and fc1.in_features % 4 == 0 and fc1.out_features % 4 == 0
            and fc2.out_features % 4 == 0 and fc1.bias is not None and fc2.bias is not None and fc3.bias is not None):
        raise _lib.PapcError("tnet_fc: float32 rows [B, Cin] and Linear layers with biases and hidden widths % 4 == 0 expected")
    if fc3.out_features % 4 == 0:
        return _head.plain_head(spec, x, fc1, fc2, _NO_DROPOUT, fc3, training=False)
    params = (fc1.weight, fc1.bias, fc2.weight, fc2.bias, fc3.weight, fc3.bias)
    spec.grad_targets = None        # (the padded node hands autograd every gradient: a [Cout, Cin] target cannot take a padded dW3)
    outs = [_HeadPlainPadded.apply(spec, 0.0, xc, *params) for xc, _ in _head._row_chunks(x, None, False)]
    return outs[0] if len(outs) == 1 else torch.cat(outs, 0)
