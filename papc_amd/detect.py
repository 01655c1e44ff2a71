"""PointPillars ``predict()``: decode, score, top-k and NMS for a whole batch on the device (csrc/detpost.hip).

Mirrors the non-multiclass path of ``PointPillars.predict`` (pointpillars/models/detectors/pointpillars.py:218-398) with ``second_box_decode``,
``center_to_corner_box2d``, ``corner_to_standup_nd``, ``nms`` and ``rotate_nms`` of libs/ops/box_paddle_ops.py.  ``predict_tensors`` is one launch
sequence for the batch -- score, one key sort, gather + decode of the first min(passing, nms_pre_max_size) ranks, suppression words, sweep + emit
-- with no host synchronisation: the counts stay on the device and the outputs are padded to ``nms_post_max_size`` rows per frame.  ``predict``
wraps it in the source's list of dicts with ONE host read (``num_det``) for the batch.

One order serves the top-k cut and the NMS sweep: descending score, and on exactly equal scores descending anchor index (what
``argsort()[::-1]`` gives, the order of ``nms.nms_gpu``).  ``paddle.topk`` leaves ties unspecified; this is the project's choice, and it replaces
the second sort inside ``nms_gpu``.  Equal class scores give the lowest label; ``dir[0] == dir[1]`` gives direction label 0.

Where the source does not run as written, the intent is taken:
  * ``paddle.argmax(dir_preds, axis=-1)[1]`` (:257) means the argmax over the last axis;
  * ``paddle.max(total_scores, axis=-1)`` unpacked into two names (:326) means (max, argmax);
  * ``a_mask.astype("int64")`` used as an index (:250-256) means a boolean mask;
  * the ``multiclass_nms`` branch (:279-318) cannot run (``selected_scores`` is never filled, the concatenation sits inside the loop): it is
    not built and ``predict`` raises for it.

``PAPC_DET_POST=0`` (environment, read once at import, as PAPC_DET_LOSS is) runs the second flavour instead: the source's op sequence in torch
device ops, frame by frame, on ``nms.nms_gpu_tensor`` / ``nms.rotate_nms_gpu_tensor``, under the same tie rule.  It synchronises with the host
as the source does; it is the A/B leg and the fallback for shapes the fused path refuses (nms_pre_max_size > 4096, more than 16 class columns).
"""
import ctypes
import math

import torch

from . import _lib, boxcodec
from . import nms as _nms
from .boxcodec import _decode_torch
from ._lib import c_p, c_f, check, ptr, stream_ptr


class DetPostDesc(ctypes.Structure):
    """papc_det_post_desc"""
    _fields_ = [("B", ctypes.c_int32), ("A", ctypes.c_int32), ("num_cls", ctypes.c_int32), ("score_mode", ctypes.c_int32),
                ("use_dir", ctypes.c_int32), ("use_rotate_nms", ctypes.c_int32), ("encode_angle_to_vector", ctypes.c_int32),
                ("smooth_dim", ctypes.c_int32),
                ("code_size", ctypes.c_int32), ("pre_max", ctypes.c_int32), ("post_max", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("score_thresh", c_f), ("iou_thresh", c_f), ("anchor_batch_stride", ctypes.c_int64)]


class DetPostIo(ctypes.Structure):
    """papc_det_post_io"""
    _fields_ = [("box_preds", c_p), ("cls_preds", c_p), ("dir_preds", c_p), ("anchors", c_p), ("anchors_mask", c_p),
                ("boxes", c_p), ("scores", c_p), ("labels", c_p), ("dir_labels", c_p), ("anchor_idx", c_p), ("num_det", c_p), ("num_pass", c_p)]


_DET_POST = _lib.env_switch("PAPC_DET_POST")                     # A/B switch: 0 = the source's op sequence in torch ops

OUTPUTS = (("boxes", torch.float32, (7,)), ("scores", torch.float32, ()), ("labels", torch.int32, ()), ("dir_labels", torch.int32, ()),
           ("anchor_idx", torch.int32, ()))


def fused_enabled():
    """what PAPC_DET_POST selected"""
    return _DET_POST


def second_box_decode(box_encodings, anchors, encode_angle_to_vector=False, smooth_dim=False, fused=None):
    """box_paddle_ops.py:48: box_encodings [..., 7] ([..., 8] with encode_angle_to_vector), anchors [..., 7] -> boxes [..., 7] (x, y, z, w, l, h, r);
    boxcodec.second_box_decode under this module's switch."""
    return boxcodec.second_box_decode(box_encodings, anchors, encode_angle_to_vector, smooth_dim, fused_enabled() if fused is None else fused)


def _score_mode(encode_background_as_zeros, use_sigmoid_score):
    if encode_background_as_zeros:
        assert use_sigmoid_score is True, "encode_background_as_zeros does not support softmax (:259-260)"
        return 0
    return 1 if use_sigmoid_score else 2


def workspace_bytes(B, A, num_cls, nms_pre_max_size, nms_post_max_size, score_mode=0, encode_angle_to_vector=False):
    """bytes of workspace one predict_tensors call of this shape needs (papc_det_post_workspace); raises PapcError outside the kernels' limits"""
    d = DetPostDesc(B=B, A=A, num_cls=num_cls, score_mode=score_mode, encode_angle_to_vector=int(bool(encode_angle_to_vector)),
                    code_size=8 if encode_angle_to_vector else 7, pre_max=nms_pre_max_size, post_max=nms_post_max_size)
    return _lib.workspace_bytes("papc_det_post_workspace", d)


def _torch_frame(box, cls, dirp, anc, mask, mode, thresh, use_dir, rotate, K, P, iou, angle_vec, smooth):
    """One frame of the source's loop body (:250-374) in torch ops under the tie rule; returns (boxes, scores, labels, dir_labels, idx, num_pass)."""
    box = _decode_torch(box, anc, angle_vec, smooth)                     # decode_paddle (:241)
    idx = torch.arange(box.shape[0], device=box.device)
    if mask is not None:
        m = mask != 0
        box, cls, idx = box[m], cls[m], idx[m]
        dirp = dirp[m] if use_dir else None
    if mode == 0:
        total = torch.sigmoid(cls)
    elif mode == 1:
        total = torch.sigmoid(cls)[..., 1:]
    else:
        total = torch.softmax(cls, dim=-1)[..., 1:]
    top = total.max(dim=-1).values
    cols = torch.arange(total.shape[-1], device=box.device).expand_as(total)
    lab = torch.where(total == top[..., None], cols, total.shape[-1]).min(dim=-1).values        # lowest class on exactly equal scores
    dl = (dirp[..., 1] > dirp[..., 0]).to(torch.int64) if use_dir else torch.zeros_like(lab)
    if thresh > 0.0:
        keep = top >= torch.tensor([thresh], dtype=top.dtype, device=top.device)
        box, top, lab, dl, idx = box[keep], top[keep], lab[keep], dl[keep], idx[keep]
    n_pass = int(top.shape[0])
    empty = (box[:0], top[:0], lab[:0], dl[:0], idx[:0], n_pass)
    if n_pass == 0:
        return empty
    order = torch.argsort(top, stable=True).flip(0)[:min(n_pass, K)]     # descending score, higher anchor first on equal scores
    box, top, lab, dl, idx = box[order], top[order], lab[order], dl[order], idx[order]
    nb = box[:, [0, 1, 3, 4, 6]]
    if not rotate:                                                       # center_to_corner_box2d -> corner_to_standup_nd
        cn = torch.tensor([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]], dtype=nb.dtype, device=nb.device)
        c = nb[:, None, 2:4] * cn[None]
        s, co = torch.sin(nb[:, 4])[:, None], torch.cos(nb[:, 4])[:, None]
        cx = c[..., 0] * co + c[..., 1] * s + nb[:, 0:1]
        cy = c[..., 0] * -s + c[..., 1] * co + nb[:, 1:2]
        nb = torch.stack([cx.min(1).values, cy.min(1).values, cx.max(1).values, cy.max(1).values], dim=1)
    # the NMS drivers sort once more (descending score, higher row first on equal scores): rows handed over in reverse rank order come back in rank order
    dets = torch.cat([nb, top[:, None]], dim=1).flip(0).contiguous()
    sel = (_nms.rotate_nms_gpu_tensor if rotate else _nms.nms_gpu_tensor)(dets, iou)
    sel = (dets.shape[0] - 1 - sel)[:P]
    box, top, lab, dl, idx = box[sel], top[sel], lab[sel], dl[sel], idx[sel]
    if use_dir:
        opp = (box[..., -1] > 0) ^ dl.bool()
        box = box.clone()
        box[..., -1] += torch.where(opp, torch.tensor(math.pi, dtype=box.dtype, device=box.device), torch.tensor(0.0, dtype=box.dtype, device=box.device))
    return box, top, lab, dl, idx, n_pass


def predict_tensors(box_preds, cls_preds, dir_cls_preds, anchors, anchors_mask=None, *, num_class, encode_background_as_zeros=True,
                    use_sigmoid_score=True, use_direction_classifier=True, use_rotate_nms=True, nms_score_threshold, nms_pre_max_size,
                    nms_post_max_size, nms_iou_threshold, encode_angle_to_vector=False, smooth_dim=False, fused=None, workspace=None, out=None):
    """The batch's detections as padded tensors.  box_preds [B,A,7|8], cls_preds [B,A,num_class (+1)], dir_cls_preds [B,A,2] (or the RPN's
    [B,H,W,.] maps, reshaped as predict() does :235-245), anchors [B,A,7] (any [B,...,7]) or one shared [A,7], anchors_mask [B,A] or None.
    Returns a dict: boxes [B,P,7], scores [B,P], labels / dir_labels / anchor_idx [B,P] int32, num_det [B], num_pass [B] int32 (anchors over
    the threshold, before the top-k cut); rows >= num_det[b] are zeros, anchor_idx -1 there.  anchor_idx counts in the unmasked numbering.
    ``workspace`` (uint8, >= workspace_bytes(...)) and ``out`` (a dict of the output tensors) may be passed in for reuse.  No host
    synchronisation on the fused path.  ``fused``: None = as PAPC_DET_POST says, False = the torch-op flavour, True = the kernels."""
    B = int(box_preds.shape[0])
    code = 8 if encode_angle_to_vector else 7
    ncls = num_class if encode_background_as_zeros else num_class + 1
    mode = _score_mode(encode_background_as_zeros, use_sigmoid_score)
    box = box_preds.reshape(B, -1, code)
    cls = cls_preds.reshape(B, -1, ncls)
    A = int(box.shape[1])
    assert cls.shape[1] == A, "box_preds and cls_preds disagree on the anchor count"
    dirp = dir_cls_preds.reshape(B, -1, 2) if use_direction_classifier else None
    shared = anchors.dim() == 2
    anc = anchors.reshape(A, 7) if shared else anchors.reshape(B, -1, 7)
    assert anc.shape[-2] == A, "anchors and box_preds disagree on the anchor count"
    mask = None if anchors_mask is None else anchors_mask.reshape(B, A)
    K, P = int(nms_pre_max_size), int(nms_post_max_size)
    dev = box.device
    use_fused = fused_enabled() if fused is None else fused
    if use_fused and not (box.is_cuda and cls.is_cuda and anc.is_cuda):
        raise _lib.PapcError("predict needs CUDA (ROCm) tensors: there is no CPU fallback (PAPC_DET_POST=0 selects the torch-op flavour)")
    res = _lib.outputs({} if out is None else out, [(name, dt, (B, P) + tail) for name, dt, tail in OUTPUTS]
                       + [("num_det", torch.int32, (B,)), ("num_pass", torch.int32, (B,))], dev)

    if not use_fused:
        box, cls, anc = box.float(), cls.float(), anc.float()
        res["boxes"].zero_(), res["scores"].zero_(), res["labels"].zero_(), res["dir_labels"].zero_(), res["anchor_idx"].fill_(-1)
        for b in range(B):
            r = _torch_frame(box[b], cls[b], dirp[b].float() if dirp is not None else None, anc if shared else anc[b],
                             None if mask is None else mask[b], mode, float(nms_score_threshold), bool(use_direction_classifier),
                             bool(use_rotate_nms), K, P, float(nms_iou_threshold), bool(encode_angle_to_vector), bool(smooth_dim))
            n = int(r[0].shape[0])
            res["boxes"][b, :n], res["scores"][b, :n] = r[0], r[1]
            res["labels"][b, :n], res["dir_labels"][b, :n], res["anchor_idx"][b, :n] = r[2].int(), r[3].int(), r[4].int()
            res["num_det"][b], res["num_pass"][b] = n, r[5]
        return res

    box, cls, anc = box.contiguous().float(), cls.contiguous().float(), anc.contiguous().float()
    if dirp is not None:
        dirp = dirp.contiguous().float()
    if mask is not None:
        mask = (mask != 0).to(torch.uint8).contiguous()
    lib = _lib.load()
    d = DetPostDesc(B=B, A=A, num_cls=ncls, score_mode=mode, use_dir=int(bool(use_direction_classifier)), use_rotate_nms=int(bool(use_rotate_nms)),
                    encode_angle_to_vector=int(bool(encode_angle_to_vector)), smooth_dim=int(bool(smooth_dim)), code_size=code, pre_max=K,
                    post_max=P, score_thresh=float(nms_score_threshold), iou_thresh=float(nms_iou_threshold),
                    anchor_batch_stride=0 if shared else A * 7)
    ws, _ = _lib.workspace("papc_det_post_workspace", d, dev, workspace)
    io = DetPostIo(box_preds=ptr(box), cls_preds=ptr(cls), dir_preds=ptr(dirp), anchors=ptr(anc), anchors_mask=ptr(mask),
                   boxes=ptr(res["boxes"]), scores=ptr(res["scores"]), labels=ptr(res["labels"]), dir_labels=ptr(res["dir_labels"]),
                   anchor_idx=ptr(res["anchor_idx"]), num_det=ptr(res["num_det"]), num_pass=ptr(res["num_pass"]))
    check(lib.papc_det_post_f32(ctypes.byref(d), ctypes.byref(io), ptr(ws), ws.numel(), stream_ptr()), "papc_det_post_f32")
    return res


def predict(example, preds_dict, *, multiclass_nms=False, **kw):
    """PointPillars.predict (:218-398): example {"anchors" [B,...,7], "image_idx" [B], "anchors_mask" (optional)}, preds_dict {"box_preds",
    "cls_preds", "dir_cls_preds"} and predict_tensors' keywords -> the source's list of dicts, one per frame: box3d_lidar [n,7], scores [n],
    label_preds [n] int64, image_idx, bbox / box3d_camera None; a frame without a detection has None entries.  One host read (num_det)."""
    if multiclass_nms:
        raise _lib.PapcError("predict: multiclass_nms is not built -- the source's branch (:279-318) cannot run as written")
    r = predict_tensors(preds_dict["box_preds"], preds_dict["cls_preds"], preds_dict.get("dir_cls_preds"), example["anchors"],
                        example.get("anchors_mask"), **kw)
    counts = r["num_det"].tolist()
    out = []
    for b, n in enumerate(counts):
        img = example["image_idx"][b]
        if n > 0:
            out.append({"bbox": None, "box3d_camera": None, "box3d_lidar": r["boxes"][b, :n], "scores": r["scores"][b, :n],
                        "label_preds": r["labels"][b, :n].to(torch.int64), "image_idx": img})
        else:
            out.append({"bbox": None, "box3d_camera": None, "box3d_lidar": None, "scores": None, "label_preds": None, "image_idx": img})
    return out
