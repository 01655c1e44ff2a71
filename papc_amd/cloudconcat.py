"""relu(bn(conv(concat([point_rows, tile(global_feat, N)])))) on the library's kernels, written once for both kernel families.

The tiled half is the same for every point of a cloud: y = x_p . W_p^T + c[b], c[b] = W_g . g[b] + bias (csrc/cloud_concat.h), so neither the
[B*N, Cp + Cg] tile nor its gradient is formed.  Then papc_bn_finalize_f32 (train mode; the running statistics get paddle's momentum rule, 0.9)
or papc_bn_eval_consts_f32 (eval mode) and papc_bn_relu_f32.  A Family names the entry points of one kernel family and says which widths it
takes: segment.py holds the Cp = 64 one (csrc/cloud_concat.hip), vfe.py the K-looped one (csrc/cloud_concat_k.hip).  Widths a family refuses,
and a caller's A/B switch set to 0, materialise the concat with copyops.cat_copy and run it as a one-layer shared-MLP stack (mlp.shared_mlp_max,
pool=False): a second, independent implementation that the tests compare against and the benchmarks' baseline.
"""
from collections import namedtuple

import torch

from . import _lib
from ._lib import BwdDy, check, cst_ptrs, ptr, stream_ptr
from .nodeparts import bn_bwd_sums

MOMENTUM = 0.9                                                # paddle's BatchNorm momentum (r = 0.9 r + 0.1 batch), as every norm here

# the C entry points of one kernel family by name, and kernel_ok(cp, cg, cout): whether the family takes a layer of these widths
Family = namedtuple("Family", "parts fwd bwd_workspace bwd kernel_ok")


class _CloudConcatBnRelu(torch.autograd.Function):
    """apply(family, x [M, Cp], g [B, Cg], w [Cout, Cp + Cg], bias, gamma, beta, running_mean, running_var, N, eps, training) -> z [M, Cout]"""

    @staticmethod
    def forward(ctx, fam, x, g, w, b, gamma, beta, rm, rv, N, eps, training):
        lib = _lib.load()
        st = stream_ptr()
        M, cp = x.shape
        B, cg = g.shape
        cout = w.shape[0]
        dev = x.device
        y = torch.empty(M, cout, device=dev, dtype=torch.float32)
        cvec = torch.empty(B, cout, device=dev, dtype=torch.float32)
        consts = torch.empty(4, cout, device=dev, dtype=torch.float32)       # mean, invstd, scale, shift
        mean, invstd, scale, shift = cst_ptrs(consts)
        fwd = getattr(lib, fam.fwd)
        if training:
            parts = getattr(lib, fam.parts)(B, N)
            stats = torch.empty(parts, 2, cout, device=dev, dtype=torch.float32)
            check(fwd(ptr(x), x.stride(0), ptr(g), ptr(w), ptr(b), B, N, cp, cg, cout, ptr(y), ptr(cvec), ptr(stats), st), fam.fwd)
            check(lib.papc_bn_finalize_f32(ptr(stats), parts, M, cout, ptr(gamma), ptr(beta), eps, MOMENTUM, mean, invstd, scale, shift, ptr(rm),
                                           ptr(rv), st), "papc_bn_finalize_f32")
        else:
            check(fwd(ptr(x), x.stride(0), ptr(g), ptr(w), ptr(b), B, N, cp, cg, cout, ptr(y), ptr(cvec), None, st), fam.fwd)
            check(lib.papc_bn_eval_consts_f32(ptr(rm), ptr(rv), ptr(gamma), ptr(beta), eps, cout, mean, invstd, scale, shift, st),
                  "papc_bn_eval_consts_f32")
        z = torch.empty(M, cout, device=dev, dtype=torch.float32)
        check(lib.papc_bn_relu_f32(ptr(y), scale, shift, M, cout, ptr(z), st), "papc_bn_relu_f32")
        ctx.save_for_backward(x, g, w, y, consts)
        ctx.fam = fam
        ctx.dims = (B, N, cp, cg, cout)
        ctx.eval_bn = not training
        ctx.has_bias = b is not None
        return z

    @staticmethod
    def backward(ctx, gz):
        x, g, w, y, consts = ctx.saved_tensors
        B, N, cp, cg, cout = ctx.dims
        fam = ctx.fam
        M = B * N
        lib = _lib.load()
        st = stream_ptr()
        dev = y.device
        gz = gz.contiguous().float()
        bn_g = torch.empty(4, cout, device=dev, dtype=torch.float32)         # dgamma, dbeta, c1, c2
        dy = BwdDy()
        dy.dz_mode, dy.dz, dy.K = 0, ptr(gz), 1
        dy.set_bn(y, consts, bn_g[2:])
        bn_bwd_sums(dy, M, cout, bn_g[2:], ptr(bn_g[0]), ptr(bn_g[1]), eval_bn=ctx.eval_bn)
        dx = torch.empty(M, cp, device=dev, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        dg = torch.empty(B, cg, device=dev, dtype=torch.float32) if ctx.needs_input_grad[2] else None
        dw = torch.empty(cout, cp + cg, device=dev, dtype=torch.float32)
        db = torch.empty(cout, device=dev, dtype=torch.float32) if ctx.has_bias else None
        nbytes = getattr(lib, fam.bwd_workspace)(B, N, cp, cg, cout)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        check(getattr(lib, fam.bwd)(ptr(gz), ptr(y), dy.mean, dy.invstd, dy.scale, dy.shift, dy.c1, dy.c2, ptr(x), x.stride(0), ptr(g), ptr(w), B, N,
                                    cp, cg, cout, ptr(dx), cp, 0, ptr(dw), ptr(db), ptr(dg), None, ptr(ws), nbytes, st), fam.bwd)
        return None, dx, dg, dw, db, bn_g[0], bn_g[1], None, None, None, None, None


def concat_bn_relu(name, family, enabled, point_rows, global_feat, conv, bn, N, training):
    """point_rows [B*N, Cp] (point-major), global_feat [B, Cg], conv = nn.Conv1d(Cp + Cg, Cout, 1) (its [Cout, Cp + Cg, 1] weight read in place),
    bn = its nn.BatchNorm1d(Cout) -> relu(bn(conv(concat([point, tile(global, N)])))) [B*N, Cout], on `family`'s kernels where `enabled` and the
    family takes the widths.  Gradients reach point_rows, global_feat, conv.weight / bias and bn.weight / bias; training=True updates bn's running
    statistics.  `name` is the public function's, for the error texts."""
    for t in (point_rows, global_feat):
        if not t.is_cuda:
            raise _lib.PapcError("%s needs CUDA (ROCm) tensors: there is no CPU fallback" % name)
        if t.dtype != torch.float32:
            raise _lib.PapcError("%s takes float32 tensors, got %s" % (name, t.dtype))
    B, cg = global_feat.shape
    cp = point_rows.shape[1]
    cout = conv.out_channels
    if point_rows.dim() != 2 or point_rows.shape[0] != B * N or conv.in_channels != cp + cg:
        raise _lib.PapcError("%s: point rows [B*N, Cp] = [%d, %d] and a conv of Cp + Cg = %d inputs expected, got %s and %d"
                             % (name, B * N, cp, cp + cg, tuple(point_rows.shape), conv.in_channels))
    if enabled and family.kernel_ok(cp, cg, cout):
        x = point_rows if (point_rows.stride(1) == 1 and point_rows.stride(0) % 4 == 0 and point_rows.data_ptr() % 16 == 0) else point_rows.contiguous()
        w2 = conv.weight.view(cout, cp + cg)
        return _CloudConcatBnRelu.apply(family, x, global_feat.contiguous(), w2, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                        int(N), float(bn.eps), bool(training))
    from .copyops import cat_copy
    from .mlp import StackSpec, shared_mlp_max
    tile = global_feat.view(B, 1, cg).expand(B, N, cg)
    rows = cat_copy([point_rows.view(B, N, cp), tile], 2).view(B * N, cp + cg)
    spec = StackSpec(B, N, 1, N, 0, xyz_first=True, eps=bn.eps, momentum=MOMENTUM, pool=False, eval_bn=not training)
    return shared_mlp_max(spec, [(bn.running_mean, bn.running_var)], None, None, None, None, [conv.weight, conv.bias, bn.weight, bn.bias], x_rows=rows)
