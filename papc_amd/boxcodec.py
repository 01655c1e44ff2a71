"""The SECOND box code, both directions: ``second_box_encode`` (libs/ops/box_np_ops.py:30-66) and its inverse ``second_box_decode``
(libs/ops/box_paddle_ops.py:48-83), each as the elementwise kernel of csrc/box_codec.h and as the source's op sequence in torch ops.
``fused`` is the caller's decision here: the public names are ``targets.second_box_encode``, which answers it from PAPC_DET_TARGETS, and
``detect.second_box_decode``, which answers it from PAPC_DET_POST."""
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr


def _const(value, like):
    """a 0-dim tensor on ``like``'s device: an operand, so that x / c is a division on every backend, never a product with a reciprocal"""
    return torch.tensor(value, dtype=like.dtype, device=like.device)


def _encode_torch(boxes, anchors, encode_angle_to_vector, smooth_dim):
    """second_box_encode (box_np_ops.py:30-66), op for op"""
    xa, ya, za, wa, la, ha, ra = torch.split(anchors, 1, dim=-1)
    xg, yg, zg, wg, lg, hg, rg = torch.split(boxes, 1, dim=-1)
    two = _const(2.0, boxes)
    zg = zg + hg / two
    za = za + ha / two
    diagonal = torch.sqrt(la * la + wa * wa)
    xt = (xg - xa) / diagonal
    yt = (yg - ya) / diagonal
    zt = (zg - za) / ha
    if smooth_dim:
        one = _const(1.0, boxes)
        lt, wt, ht = lg / la - one, wg / wa - one, hg / ha - one
    else:
        lt, wt, ht = torch.log(lg / la), torch.log(wg / wa), torch.log(hg / ha)
    if encode_angle_to_vector:
        return torch.cat([xt, yt, zt, wt, lt, ht, torch.cos(rg) - torch.cos(ra), torch.sin(rg) - torch.sin(ra)], dim=-1)
    return torch.cat([xt, yt, zt, wt, lt, ht, rg - ra], dim=-1)


def _decode_torch(t, a, encode_angle_to_vector, smooth_dim):
    """second_box_decode (box_paddle_ops.py:48-83), op for op"""
    xa, ya, za, wa, la, ha, ra = torch.split(a, 1, dim=-1)
    if encode_angle_to_vector:
        xt, yt, zt, wt, lt, ht, rtx, rty = torch.split(t, 1, dim=-1)
    else:
        xt, yt, zt, wt, lt, ht, rt = torch.split(t, 1, dim=-1)
    za = za + ha / 2
    diagonal = torch.sqrt(la ** 2 + wa ** 2)
    xg = xt * diagonal + xa
    yg = yt * diagonal + ya
    zg = zt * ha + za
    if smooth_dim:
        lg, wg, hg = (lt + 1) * la, (wt + 1) * wa, (ht + 1) * ha
    else:
        lg, wg, hg = torch.exp(lt) * la, torch.exp(wt) * wa, torch.exp(ht) * ha
    if encode_angle_to_vector:
        rg = torch.atan2(rty + torch.sin(ra), rtx + torch.cos(ra))
    else:
        rg = rt + ra
    zg = zg - hg / 2
    return torch.cat([xg, yg, zg, wg, lg, hg, rg], dim=-1)


def _launch(symbol, rows, anchors, code, width, encode_angle_to_vector, smooth_dim):
    """``rows`` [..., k] and ``anchors`` (broadcast to [..., 7]) through papc_box_encode_f32 / papc_box_decode_f32 -> [..., width]"""
    rows = rows.contiguous().float()
    anc = anchors.expand(rows.shape[:-1] + (7,)).contiguous().float()
    out = torch.empty(rows.shape[:-1] + (width,), dtype=torch.float32, device=rows.device)
    n = out.numel() // width
    if n:
        check(getattr(_lib.load(), symbol)(ptr(rows), ptr(anc), n, code, int(bool(encode_angle_to_vector)), int(bool(smooth_dim)), ptr(out),
                                           stream_ptr()), symbol)
    return out


def second_box_encode(boxes, anchors, encode_angle_to_vector, smooth_dim, fused):
    """box_np_ops.py:30: boxes [..., 7] (x, y, z, w, l, h, r), anchors [..., 7] -> encodings [..., 7] ([..., 8] with encode_angle_to_vector);
    the inverse of second_box_decode."""
    assert boxes.shape[-1] == 7 and anchors.shape[-1] == 7, "boxes [..., 7] and anchors [..., 7] expected"
    if not fused:
        return _encode_torch(boxes.float(), anchors.float().expand(boxes.shape), encode_angle_to_vector, smooth_dim)
    if not boxes.is_cuda or not anchors.is_cuda:
        raise _lib.PapcError("second_box_encode needs CUDA (ROCm) tensors: there is no CPU fallback (PAPC_DET_TARGETS=0 selects the torch-op flavour)")
    code = 8 if encode_angle_to_vector else 7
    return _launch("papc_box_encode_f32", boxes, anchors, code, code, encode_angle_to_vector, smooth_dim)


def second_box_decode(box_encodings, anchors, encode_angle_to_vector, smooth_dim, fused):
    """box_paddle_ops.py:48: box_encodings [..., 7] ([..., 8] with encode_angle_to_vector), anchors [..., 7] -> boxes [..., 7] (x, y, z, w, l, h, r);
    the inverse of second_box_encode."""
    code = 8 if encode_angle_to_vector else 7
    assert box_encodings.shape[-1] == code and anchors.shape[-1] == 7, "box_encodings [..., %d] and anchors [..., 7] expected" % code
    if not fused:
        return _decode_torch(box_encodings, anchors.expand(box_encodings.shape[:-1] + (7,)), encode_angle_to_vector, smooth_dim)
    if not box_encodings.is_cuda or not anchors.is_cuda:
        raise _lib.PapcError("second_box_decode needs CUDA (ROCm) tensors: there is no CPU fallback (PAPC_DET_POST=0 selects the torch-op flavour)")
    return _launch("papc_box_decode_f32", box_encodings, anchors, code, 7, encode_angle_to_vector, smooth_dim)
