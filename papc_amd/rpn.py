"""The PointPillars RPN on the library's kernels: a dense 2-D CNN over the pillar canvas.

Reference: PAPC/models/detect/pointpillars/models/bones/rpn.py:8-170
    three blocks, each Pad2D(1) + Conv2D(3, stride s) and layer_nums[i] x Conv2D(3, padding=1), every conv + BatchNorm2D(eps 1e-3, momentum
    0.01) + ReLU; three Conv2DTranspose(kernel = stride) + BatchNorm + ReLU; channel concat; conv_box / conv_cls / conv_dir_cls (1x1, bias);
    outputs transposed to [B, H, W, .].
csrc/conv2d.hip runs every conv and deconv as an implicit GEMM on the bf16x3 matrix-pipe bodies over channel-last rows [B H W, C] of the
PRE-norm output: the norm and the ReLU are applied by the consumer on load, the statistics come from the producer's epilogue, the three
deconvs write straight into the [B H1 W1, sum Cup] concat buffer, and the backward recomputes every ReLU sign.  ``_RPNBackbone`` is ONE autograd
node over those launches (canvas -> activated concat rows); it keeps the canvas rows, each layer's pre-norm y, the norm constants and the
weights in the dX kernels' K-major order -- never a mask or an activated copy.  The heads are one fused row GEMM (linear.linear_rows) split
into three column views: the source's final transposes are free.

Paddle semantics: ``momentum`` is the weight of the RUNNING value, running <- 0.01 running + 0.99 batch, with the biased batch variance.

PAPC_RPN=0 (read once, at import) runs the same module in torch device ops instead -- each conv an im2col view and a matmul, no
convolution-library call: a second, independent implementation the tests compare against and the baseline of tools/bench_rpn.py.  It also
takes over for use_norm=False, shapes outside papc_conv2d_ok, an eval-mode forward that records gradients, non-float32 and CPU tensors.
"""
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import check, ptr, stream_ptr
from .nodeparts import all_or_none, grad_targets_of

_RPN = os.environ.get("PAPC_RPN", "1") != "0"                # A/B switch: 0 = the module in torch device ops
BN_MOMENTUM = 0.01           # rpn.py:46: paddle's momentum, the weight of the RUNNING value
BN_EPS = 1e-3


class _Layer:
    """one conv or deconv of the backbone as the node sees it"""

    def __init__(self, conv, bn, deconv, stride, src):
        self.conv, self.bn, self.deconv, self.stride, self.src = conv, bn, deconv, stride, src   # src: the producer's index, -1 = the canvas
        w = conv.weight
        self.cin, self.cout = (w.shape[0], w.shape[1]) if deconv else (w.shape[1], w.shape[0])


def _cst4(cst):
    return _lib.cst_ptrs(cst)


class _RPNBackbone(torch.autograd.Function):
    """apply(grad targets or None, layers (list of _Layer: the block convs in order, then the three deconvs), block ends (index of each block's
    last conv), training, canvas [B, C, H, W], *(w, gamma, beta per layer)) -> the activated concat rows [B H1 W1, sum Cup].
    Saved: the canvas rows, every layer's pre-norm y (the deconvs': the concat buffer), the constants [4, C] per layer, wt per layer."""

    @staticmethod
    def forward(ctx, targets, layers, ends, training, canvas, *params):
        lib, st, dev = _lib.load(), stream_ptr(), canvas.device
        B, C0, H, W = canvas.shape
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)      # noqa: E731
        n = len(layers)
        ws = [params[3 * i] for i in range(n)]
        # the canvas as rows [B H W, C]: one strided copy
        x0 = new(B * H * W, C0)
        cv = canvas.view(B, C0, H * W).transpose(1, 2)
        job = _lib.CopyJob(cv.data_ptr(), x0.data_ptr(), B, H * W, C0, *cv.stride(), H * W * C0, C0, 1)
        check(lib.papc_copy_strided_batch_f32((_lib.CopyJob * 1)(job), 1, st), "papc_copy_strided_batch_f32")
        # every weight in its two K-major orders: one launch
        wk = [new(w.numel()) for w in ws]
        wt = [new(w.numel()) for w in ws]
        arr_p, arr_i = ctypes.c_void_p * n, ctypes.c_int * n
        check(lib.papc_conv2d_prep_f32(arr_p(*[w.data_ptr() for w in ws]), arr_p(*[t.data_ptr() for t in wk]), arr_p(*[t.data_ptr() for t in wt]),
                                       arr_i(*[l.cin for l in layers]), arr_i(*[l.cout for l in layers]), arr_i(*[l.stride for l in layers]),
                                       arr_i(*[int(l.deconv) for l in layers]), n, st), "papc_conv2d_prep_f32")
        nconv = n - 3
        cup = [l.cout for l in layers[nconv:]]
        ys, csts, geo = [None] * n, [None] * n, [None] * n          # geo: (H, W) of the layer's INPUT
        cstup = new(4, sum(cup))
        hw = [(H, W)] * n                                            # (H, W) of the layer's OUTPUT

        def norm(i, part, parts, M, cst):
            l = layers[i]
            g, b = params[3 * i + 1], params[3 * i + 2]
            if training:
                check(lib.papc_bn_finalize_f32(ptr(part), parts, M, l.cout, ptr(g), ptr(b), l.bn.eps, BN_MOMENTUM, *_cst4(cst), ptr(l.bn.running_mean),
                                               ptr(l.bn.running_var), st), "papc_bn_finalize_f32")
            else:
                check(lib.papc_bn_eval_consts_f32(ptr(l.bn.running_mean), ptr(l.bn.running_var), ptr(g), ptr(b), l.bn.eps, l.cout, *_cst4(cst), st),
                      "papc_bn_eval_consts_f32")

        for i in range(nconv):
            l = layers[i]
            h, w = (H, W) if l.src < 0 else hw[l.src]
            x = x0 if l.src < 0 else ys[l.src]
            sc, sh = (0, 0) if l.src < 0 else _cst4(csts[l.src])[2:]
            ho, wo = (h - 1) // l.stride + 1, (w - 1) // l.stride + 1
            M = B * ho * wo
            parts = lib.papc_conv2d_parts(M)
            y, part, cst = new(M, l.cout), new(parts, 2, l.cout), new(4, l.cout)
            check(lib.papc_conv2d_fwd_f32(ptr(x), sc, sh, ptr(wk[i]), B, h, w, l.cin, l.cout, l.stride, ptr(y), ptr(part), st), "papc_conv2d_fwd_f32")
            norm(i, part, parts, M, cst)
            ys[i], csts[i], geo[i], hw[i] = y, cst, (h, w), (ho, wo)
        # the three deconvs into the concat buffer
        h1, w1 = hw[ends[0]][0] * layers[nconv].stride, hw[ends[0]][1] * layers[nconv].stride
        M1 = B * h1 * w1
        ycat = new(M1, sum(cup))
        coff = 0
        for k in range(3):
            i = nconv + k
            l = layers[i]
            h, w = hw[l.src]
            if (h * l.stride, w * l.stride) != (h1, w1):
                raise _lib.PapcError("RPN: the upsampled maps differ in size (%d x %d against %d x %d): the canvas does not divide by the strides"
                                     % (h * l.stride, w * l.stride, h1, w1))
            parts = lib.papc_conv2d_parts(B * h * w) * l.stride ** 2
            part = new(parts, 2, l.cout)
            check(lib.papc_deconv2d_fwd_f32(ptr(ys[l.src]), *_cst4(csts[l.src])[2:], ptr(wk[i]), B, h, w, l.cin, l.cout, l.stride, ptr(ycat), sum(cup), coff,
                                            ptr(part), st), "papc_deconv2d_fwd_f32")
            csts[i] = cstup[:, coff:coff + l.cout]
            norm(i, part, parts, M1, csts[i])
            geo[i], hw[i] = (h, w), (h1, w1)
            coff += l.cout
        out = new(M1, sum(cup))
        check(lib.papc_bn_relu_f32(ptr(ycat), ptr(cstup[2]), ptr(cstup[3]), M1, sum(cup), ptr(out), st), "papc_bn_relu_f32")
        ctx.save_for_backward(x0, ycat, cstup, *ys[:nconv], *csts[:nconv], *wt)
        ctx.layers, ctx.ends, ctx.targets, ctx.dims, ctx.geo, ctx.hw, ctx.training = layers, ends, targets, (B, C0, H, W), geo, hw, training
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, gout):
        layers, ends, geo = ctx.layers, ctx.ends, ctx.geo
        n = len(layers)
        nconv = n - 3
        saved = ctx.saved_tensors
        x0, ycat, cstup = saved[:3]
        ys, csts, wt = list(saved[3:3 + nconv]), list(saved[3 + nconv:3 + 2 * nconv]), saved[3 + 2 * nconv:]
        if gout is None:
            return (None,) * (5 + 3 * n)
        B, C0, H, W = ctx.dims
        lib, st, dev = _lib.load(), stream_ptr(), x0.device
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)      # noqa: E731
        gout = gout.contiguous().float()
        shapes = []
        for l in layers:
            shapes += [tuple(l.conv.weight.shape), (l.cout,), (l.cout,)]
        tg, acc, grads = all_or_none(ctx.targets, shapes, dev)
        fin = acc | (0 if ctx.training else 2)
        cup = [l.cout for l in layers[nconv:]]
        ld = sum(cup)
        M1 = ycat.shape[0]
        c12 = [new(2, l.cout) for l in layers]
        dzs = [None] * nconv

        def c12p(i):
            return c12[i].data_ptr(), c12[i].data_ptr() + 4 * c12[i].stride(0)

        def finalize(i, red, M):
            check(lib.papc_bn_bwd_finalize_f32(ptr(red), red.shape[0], M, layers[i].cout, ptr(tg[3 * i + 1]), ptr(tg[3 * i + 2]), *c12p(i), fin, st),
                  "papc_bn_bwd_finalize_f32")

        def prev_of(i):
            """the producer under layer i's dX epilogue: (y_prev, mean, invstd, scale, shift, dz_prev, red) or the canvas"""
            src = layers[i].src
            h, w = geo[i]
            if src < 0:
                return (0, 0, 0, 0, 0), new(B * h * w, layers[i].cin), None
            red = new(lib.papc_conv2d_parts(B * h * w), 2, layers[i].cin)
            return (ptr(ys[src]),) + tuple(_cst4(csts[src])), new(B * h * w, layers[i].cin), red

        def dw_of(i, dz, y, ldy, coff, cst):
            l = layers[i]
            h, w = geo[i]
            x = x0 if l.src < 0 else ys[l.src]
            sc, sh = (0, 0) if l.src < 0 else _cst4(csts[l.src])[2:]
            m, s_, sc_ = cst[0], cst[1], cst[2]
            if l.deconv:
                nb = lib.papc_deconv2d_bwd_dw_workspace(B, h, w, l.cin, l.cout, l.stride)
                wsb = torch.empty(nb, device=dev, dtype=torch.uint8)
                check(lib.papc_deconv2d_bwd_dw_f32(ptr(dz), ptr(y), ldy, coff, m, s_, sc_, *c12p(i), ptr(x), sc, sh, B, h, w, l.cin, l.cout, l.stride,
                                                   ptr(tg[3 * i]), acc, ptr(wsb), nb, st), "papc_deconv2d_bwd_dw_f32")
            else:
                nb = lib.papc_conv2d_bwd_dw_workspace(B, h, w, l.cin, l.cout, l.stride)
                wsb = torch.empty(nb, device=dev, dtype=torch.uint8)
                check(lib.papc_conv2d_bwd_dw_f32(ptr(dz), ptr(y), m, s_, sc_, *c12p(i), ptr(x), sc, sh, B, h, w, l.cin, l.cout, l.stride, ptr(tg[3 * i]), acc,
                                                 ptr(wsb), nb, st), "papc_conv2d_bwd_dw_f32")

        # the concat buffer: dz = gout x ReLU' and the deconv norms' sums, per deconv (its columns)
        dzcat = new(M1, ld)
        rparts = lib.papc_conv2d_relu_bwd_parts(M1)
        coffs, coff = [], 0
        for k in range(3):
            i = nconv + k
            cu = _cst4(cstup[:, coff:coff + cup[k]])
            red = new(rparts, 2, cup[k])
            check(lib.papc_conv2d_relu_bwd_f32(ptr(gout), ptr(ycat), ld, coff, *cu, M1, cup[k], ptr(dzcat), ptr(red), st), "papc_conv2d_relu_bwd_f32")
            finalize(i, red, M1)
            coffs.append(coff)
            coff += cup[k]
        dcanvas = None
        first = [0] + [e + 1 for e in ends[:2]]                     # each block's first conv
        for blk in (2, 1, 0):
            i = nconv + blk
            l = layers[i]
            h, w = geo[i]
            cu = _cst4(cstup[:, coffs[blk]:coffs[blk] + l.cout])
            last = ends[blk]
            if blk == 2:                                            # the deconv is the block output's only consumer
                pv, dzp, red = prev_of(i)
                check(lib.papc_deconv2d_bwd_dx_f32(ptr(dzcat), ptr(ycat), ld, coffs[blk], cu[0], cu[1], cu[2], *c12p(i), ptr(wt[i]), B, h, w, l.cin, l.cout,
                                                   l.stride, 0, *pv, ptr(dzp), ptr(red), st), "papc_deconv2d_bwd_dx_f32")
            else:                                                   # the deconv's dA rides the next block's first dX as its addend
                tmp = new(B * h * w, l.cin)
                check(lib.papc_deconv2d_bwd_dx_f32(ptr(dzcat), ptr(ycat), ld, coffs[blk], cu[0], cu[1], cu[2], *c12p(i), ptr(wt[i]), B, h, w, l.cin, l.cout,
                                                   l.stride, 0, 0, 0, 0, 0, 0, ptr(tmp), 0, st), "papc_deconv2d_bwd_dx_f32")
                j = first[blk + 1]
                lj = layers[j]
                cj = _cst4(csts[j])
                pv, dzp, red = prev_of(j)
                check(lib.papc_conv2d_bwd_dx_f32(ptr(dzs[j]), ptr(ys[j]), cj[0], cj[1], cj[2], *c12p(j), ptr(wt[j]), B, h, w, lj.cin, lj.cout, lj.stride,
                                                 ptr(tmp), *pv, ptr(dzp), ptr(red), st), "papc_conv2d_bwd_dx_f32")
                dzs[j] = None
            dzs[last] = dzp
            finalize(last, red, B * h * w)
            dw_of(i, dzcat, ycat, ld, coffs[blk], cu)
            for j in range(last, first[blk] - 1, -1):
                lj = layers[j]
                cj = _cst4(csts[j])
                dw_of(j, dzs[j], ys[j], lj.cout, 0, cj)
                if j > first[blk]:
                    hj, wj = geo[j]
                    pv, dzp, red = prev_of(j)
                    check(lib.papc_conv2d_bwd_dx_f32(ptr(dzs[j]), ptr(ys[j]), cj[0], cj[1], cj[2], *c12p(j), ptr(wt[j]), B, hj, wj, lj.cin, lj.cout, lj.stride,
                                                     0, *pv, ptr(dzp), ptr(red), st), "papc_conv2d_bwd_dx_f32")
                    dzs[j - 1] = dzp
                    finalize(j - 1, red, B * hj * wj)
                    dzs[j] = None
                elif blk == 0 and ctx.needs_input_grad[4]:          # the canvas: no norm above it
                    pv, dx0, _ = prev_of(j)
                    check(lib.papc_conv2d_bwd_dx_f32(ptr(dzs[j]), ptr(ys[j]), cj[0], cj[1], cj[2], *c12p(j), ptr(wt[j]), B, H, W, lj.cin, lj.cout, lj.stride,
                                                     0, *pv, ptr(dx0), 0, st), "papc_conv2d_bwd_dx_f32")
                    dcanvas = new(B, C0, H, W)
                    dv = dcanvas.view(B, C0, H * W).transpose(1, 2)
                    job = _lib.CopyJob(dx0.data_ptr(), dv.data_ptr(), B, H * W, C0, H * W * C0, C0, 1, *dv.stride())
                    check(lib.papc_copy_strided_batch_f32((_lib.CopyJob * 1)(job), 1, st), "papc_copy_strided_batch_f32")
        return (None, None, None, None, dcanvas) + tuple(grads)


# ---- the second path: torch device ops ------------------------------------------------------------------------------------------------------

def _conv3x3_rows(a, weight, stride):
    """a [B, H, W, Ci] (activated) -> rows [B Ho Wo, Co] of the 3x3 conv with a zero halo of 1, as an im2col view and a matmul"""
    B = a.shape[0]
    u = F.pad(a, (0, 0, 1, 1, 1, 1)).unfold(1, 3, stride).unfold(2, 3, stride)                   # [B, Ho, Wo, Ci, 3, 3]: the weight's own K order
    ho, wo = u.shape[1], u.shape[2]
    return torch.matmul(u.reshape(B * ho * wo, -1), weight.reshape(weight.shape[0], -1).t()), ho, wo


def _deconv_rows(a, weight, s):
    """a [B, H, W, Ci] -> [B, s H, s W, Co] of the kernel = stride transposed conv: a matmul and a pixel shuffle"""
    B, H, W, ci = a.shape
    co = weight.shape[1]
    y = torch.matmul(a.reshape(-1, ci), weight.reshape(ci, co * s * s)).view(B, H, W, co, s, s)
    return y.permute(0, 1, 4, 2, 5, 3).reshape(B, H * s, W * s, co)


def _norm_relu_torch(y, bn, bias, training):
    """y [..., C] rows -> relu(norm(y + bias)); the running statistics by the paddle rule (biased variance, momentum on the running value)"""
    if bias is not None:
        y = y + bias
    if isinstance(bn, nn.BatchNorm2d):
        if training:
            flat = y.reshape(-1, y.shape[-1])
            mean, var = flat.mean(0), flat.var(0, unbiased=False)
            with torch.no_grad():
                bn.running_mean.mul_(BN_MOMENTUM).add_(mean.detach(), alpha=1.0 - BN_MOMENTUM)
                bn.running_var.mul_(BN_MOMENTUM).add_(var.detach(), alpha=1.0 - BN_MOMENTUM)
        else:
            mean, var = bn.running_mean, bn.running_var
        y = (y - mean) / torch.sqrt(var + bn.eps) * bn.weight + bn.bias
    return F.relu(y)


def _is_conv(m):
    return isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))


class RPN(nn.Module):
    """rpn.py:8-170 with the source's constructor signature and module tree (block1..3 with the pad layer at index 0, deconv1..3, conv_cls,
    conv_box, conv_dir_cls: the state-dict keys are the source's).  forward(x [B, C, ny, nx]) -> {"box_preds", "cls_preds", "dir_cls_preds"}
    as [B, H, W, .].  use_groupnorm / use_bev are not built."""

    def __init__(self, use_norm=True, num_class=2, layer_nums=(3, 5, 5), layer_strides=(2, 2, 2), num_filters=(128, 128, 256),
                 upsample_strides=(1, 2, 4), num_upsample_filters=(256, 256, 256), num_input_filters=128, num_anchor_per_loc=2,
                 encode_background_as_zeros=True, use_direction_classifier=True, use_groupnorm=False, num_groups=32, use_bev=False,
                 box_code_size=7, name='rpn'):
        super().__init__()
        if use_groupnorm or use_bev:
            raise _lib.PapcError("RPN: use_groupnorm / use_bev: not built")
        if not (len(layer_nums) == len(layer_strides) == len(num_filters) == len(upsample_strides) == len(num_upsample_filters) == 3):
            raise _lib.PapcError("RPN: three blocks expected (rpn.py:30-34)")
        self._num_anchor_per_loc = num_anchor_per_loc
        self._use_direction_classifier = use_direction_classifier
        self._use_norm = use_norm
        self._strides, self._up = [int(s) for s in layer_strides], [int(s) for s in upsample_strides]
        bias = not use_norm

        def norm(c):          # torch's momentum weighs the BATCH value: 1 - paddle's
            return nn.BatchNorm2d(c, eps=BN_EPS, momentum=1.0 - BN_MOMENTUM) if use_norm else nn.Identity()

        cin = num_input_filters
        for i in range(3):
            f = num_filters[i]
            seq = [nn.ZeroPad2d(1), nn.Conv2d(cin, f, 3, stride=layer_strides[i], bias=bias), norm(f), nn.ReLU()]
            for _ in range(layer_nums[i]):
                seq += [nn.Conv2d(f, f, 3, padding=1, bias=bias), norm(f), nn.ReLU()]
            setattr(self, "block%d" % (i + 1), nn.Sequential(*seq))
            setattr(self, "deconv%d" % (i + 1), nn.Sequential(
                nn.ConvTranspose2d(f, num_upsample_filters[i], upsample_strides[i], stride=upsample_strides[i], bias=bias),
                norm(num_upsample_filters[i]), nn.ReLU()))
            cin = f
        num_cls = num_anchor_per_loc * num_class if encode_background_as_zeros else num_anchor_per_loc * (num_class + 1)
        cup = sum(num_upsample_filters)
        self.conv_cls = nn.Conv2d(cup, num_cls, 1)
        self.conv_box = nn.Conv2d(cup, num_anchor_per_loc * box_code_size, 1)
        if use_direction_classifier:
            self.conv_dir_cls = nn.Conv2d(cup, num_anchor_per_loc * 2, 1)

    # -- the layer list the node walks --
    def _layers(self):
        layers, ends = [], []
        for i in range(3):
            blk = getattr(self, "block%d" % (i + 1))
            mods = list(blk)
            convs = [k for k, m in enumerate(mods) if _is_conv(m)]
            for t, k in enumerate(convs):
                src = len(layers) - 1                               # the previous layer (block 1's first: -1, the canvas)
                layers.append(_Layer(mods[k], mods[k + 1], False, self._strides[i] if t == 0 else 1, src))
            ends.append(len(layers) - 1)
        for i in range(3):
            dc = getattr(self, "deconv%d" % (i + 1))
            layers.append(_Layer(dc[0], dc[1], True, self._up[i], ends[i]))
        return layers, ends

    def _heads(self):
        heads = [("cls_preds", self.conv_cls), ("box_preds", self.conv_box)]
        if self._use_direction_classifier:
            heads.append(("dir_cls_preds", self.conv_dir_cls))
        return heads

    def kernel_ok(self, x):
        """whether csrc/conv2d.hip takes this module on this canvas"""
        if not (self._use_norm and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            return False
        lib = _lib.load()
        layers, _ = self._layers()
        if x.shape[1] != layers[0].cin or len(layers) > 32:
            return False
        h, w = int(x.shape[2]), int(x.shape[3])
        for l in layers:
            if l.conv.weight.dtype != torch.float32:
                return False
            if l.deconv:
                if not lib.papc_deconv2d_ok(l.cin, l.cout, l.stride):
                    return False
            else:
                if not lib.papc_conv2d_ok(l.cin, l.cout, l.stride, h, w):
                    return False
                h, w = (h - 1) // l.stride + 1, (w - 1) // l.stride + 1
        return True

    def backbone_rows(self, x):
        """canvas [B, C, H, W] -> (the activated concat rows [B H1 W1, sum Cup], H1, W1)"""
        layers, ends = self._layers()
        grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if not (_RPN and self.kernel_ok(x) and (self.training or not grad)):
            return self._backbone_torch(x, layers, ends)
        params = []
        for l in layers:
            params += [l.conv.weight, l.bn.weight, l.bn.bias]
        tg = grad_targets_of(params) if torch.is_grad_enabled() else None
        rows = _RPNBackbone.apply(tg, layers, ends, bool(self.training), x.contiguous(), *params)
        s = layers[-3].stride
        h, w = int(x.shape[2]), int(x.shape[3])
        for l in layers[:ends[0] + 1]:
            h, w = (h - 1) // l.stride + 1, (w - 1) // l.stride + 1
        return rows, h * s, w * s

    def _backbone_torch(self, x, layers, ends):
        a = x.permute(0, 2, 3, 1)                                    # channel-last: every conv a matmul over rows
        B = a.shape[0]
        acts, ups = [], []
        for i, l in enumerate(layers):
            if l.deconv:
                y = _deconv_rows(acts[l.src], l.conv.weight, l.stride)
                ups.append(_norm_relu_torch(y, l.bn, l.conv.bias, self.training))
            else:
                y, ho, wo = _conv3x3_rows(a if l.src < 0 else acts[l.src], l.conv.weight, l.stride)
                acts.append(_norm_relu_torch(y.view(B, ho, wo, -1), l.bn, l.conv.bias, self.training))
        if not (ups[0].shape[1:3] == ups[1].shape[1:3] == ups[2].shape[1:3]):
            raise _lib.PapcError("RPN: the upsampled maps differ in size (%s, %s, %s): the canvas does not divide by the strides"
                                 % tuple(tuple(u.shape[1:3]) for u in ups))
        cat = torch.cat(ups, dim=3)
        return cat.reshape(-1, cat.shape[3]), cat.shape[1], cat.shape[2]

    def forward(self, x, bev=None):
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise _lib.PapcError("RPN: a canvas [B, C, ny, nx] expected")
        if x.shape[1] != self.block1[1].weight.shape[1]:
            raise _lib.PapcError("RPN: %d input channels expected, got %d" % (self.block1[1].weight.shape[1], x.shape[1]))
        B = x.shape[0]
        rows, h1, w1 = self.backbone_rows(x)
        heads = self._heads()
        wh = torch.cat([m.weight.reshape(m.weight.shape[0], -1) for _, m in heads], 0)
        bh = torch.cat([m.bias for _, m in heads], 0)
        if rows.is_cuda and rows.dtype == torch.float32 and _RPN:
            from .linear import linear_rows
            out = linear_rows(rows, wh, bh, inplace=False)           # one fused row GEMM for the three heads
        else:
            out = torch.matmul(rows, wh.t()) + bh
        ret, c0 = {}, 0
        for name, m in heads:
            c = m.weight.shape[0]
            ret[name] = out[:, c0:c0 + c].reshape(B, h1, w1, c)      # rpn.py:160-168: the transposes are free on rows
            c0 += c
        return {k: ret[k] for k in ("box_preds", "cls_preds", "dir_cls_preds") if k in ret}
