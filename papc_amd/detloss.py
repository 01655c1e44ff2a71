"""The PointPillars detection loss (pointpillars/models/detectors/pointpillars.py:150-213, 468-585 on core/losses.py) as ONE autograd node.

``pointpillars_loss`` turns the RPN's three prediction maps, the assigner's labels / regression targets and the anchors into the reference's
result dict.  The default flavour is csrc/detloss.hip: three launches (counts, main pass, fold) produce the scalar, the reduced by-products,
the per-anchor losses and -- for upstream gradient 1 -- all three gradients; the backward multiplies the stored gradients by the incoming
scalar on the device (nothing when seeded with ``head.unit_gradient``).  No ``.item()``, no host synchronisation: the node can sit inside a
captured graph.  Sums are folded in a fixed order (csrc/fold.h), so the same inputs give the same bits.

``PAPC_DET_LOSS=0`` (environment, read once at import, as PAPC_VOXNET is) runs the second flavour instead: the reference's five functions and
its loss classes restated in torch ops, under their own names and argument lists below.  They take tensors of any device and float dtype.
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import c_p, c_f, check, ptr, stream_ptr

NORM_TYPES = {"NormByNumExamples": 0, "NormByNumPositives": 1, "NormByNumPosNeg": 2}     # PAPC_DET_NORM_*


class DetLossDesc(ctypes.Structure):
    """papc_det_loss_desc"""
    _fields_ = [("B", ctypes.c_int32), ("A", ctypes.c_int32), ("C", ctypes.c_int32), ("code_size", ctypes.c_int32),
                ("norm_type", ctypes.c_int32), ("has_alpha", ctypes.c_int32), ("sin_diff", ctypes.c_int32), ("has_dir", ctypes.c_int32),
                ("encode_background_as_zeros", ctypes.c_int32), ("codewise", ctypes.c_int32), ("labels_i64", ctypes.c_int32),
                ("reserved", ctypes.c_int32),
                ("pos_cls_weight", c_f), ("neg_cls_weight", c_f), ("alpha", c_f), ("gamma", c_f), ("sigma", c_f),
                ("code_weights", c_f * 7), ("loc_weight", c_f), ("cls_weight", c_f), ("dir_weight", c_f)]


class DetLossIo(ctypes.Structure):
    """papc_det_loss_io"""
    _fields_ = [("box_preds", c_p), ("cls_preds", c_p), ("dir_preds", c_p), ("labels", c_p), ("reg_targets", c_p), ("anchors", c_p),
                ("out", c_p), ("dbox", c_p), ("dcls", c_p), ("ddir", c_p), ("cls_loss", c_p), ("loc_loss", c_p), ("cared", c_p),
                ("workspace", c_p)]


_DET_LOSS = _lib.env_switch("PAPC_DET_LOSS")                     # A/B switch: 0 = the loss in torch ops


def fused_enabled():
    """what PAPC_DET_LOSS selected"""
    return _DET_LOSS


# ---- the reference's loss classes (core/losses.py), in torch ops --------------------------------------------------------------------------

def _sigmoid_cross_entropy_with_logits(logits, labels):
    """losses.py:185-189"""
    return torch.clamp(logits, min=0) - logits * labels.to(logits.dtype) + torch.log1p(torch.exp(-torch.abs(logits)))


_ROWS = {}


def _code_weight_row(code_weights, like):
    """the code weights as a [1, 1, k] tensor beside ``like``, uploaded once per (values, device, dtype).  Under stream capture a host-to-device
    copy is not allowed and a tensor born in the capture must not be cached (_lib.const_vec): the row is then filled from scalars."""
    key = (tuple(float(v) for v in code_weights), str(like.device), like.dtype)
    t = _ROWS.get(key)
    if t is None:
        if _lib._capturing():
            return torch.stack([torch.full((), v, dtype=like.dtype, device=like.device) for v in key[0]]).reshape(1, 1, -1)
        t = _ROWS[key] = torch.tensor(key[0], dtype=like.dtype, device=like.device).reshape(1, 1, -1)
    return t


class WeightedSmoothL1LocalizationLoss:
    """losses.py:134-183"""

    def __init__(self, sigma=3.0, code_weights=None, codewise=True):
        self._sigma, self._code_weights, self._codewise = float(sigma), code_weights, codewise

    def __call__(self, prediction_tensor, target_tensor, weights=None):
        diff = prediction_tensor - target_tensor
        if self._code_weights is not None:
            diff = _code_weight_row(self._code_weights, diff) * diff
        abs_diff = torch.abs(diff)
        lt = (abs_diff <= 1.0 / self._sigma ** 2).to(abs_diff.dtype)
        loss = lt * 0.5 * torch.pow(abs_diff * self._sigma, 2) + (abs_diff - 0.5 / self._sigma ** 2) * (1.0 - lt)
        if self._codewise:
            return loss if weights is None else loss * weights.unsqueeze(-1)
        loss = loss.sum(2)
        return loss if weights is None else loss * weights


class SigmoidFocalClassificationLoss:
    """losses.py:234-292.  1 - p_t is taken as the sigmoid of the logit with the target's sign flipped (what the kernel does) instead of the
    source's subtraction from one: the same number, without the cancellation at confident logits."""

    def __init__(self, gamma=2.0, alpha=0.25):
        self._alpha, self._gamma = alpha, gamma

    def __call__(self, prediction_tensor, target_tensor, weights):
        ce = _sigmoid_cross_entropy_with_logits(prediction_tensor, target_tensor)
        loss = ce
        if self._gamma:
            one_minus_pt = torch.sigmoid(prediction_tensor * (1.0 - 2.0 * target_tensor))
            loss = (one_minus_pt * one_minus_pt if self._gamma == 2.0 else torch.pow(one_minus_pt, self._gamma)) * loss
        if self._alpha is not None:
            loss = (target_tensor * self._alpha + (1.0 - target_tensor) * (1.0 - self._alpha)) * loss
        return loss * weights.unsqueeze(2)


class WeightedSigmoidClassificationLoss(SigmoidFocalClassificationLoss):
    """losses.py:202-231: the focal loss without its two factors"""

    def __init__(self):
        super().__init__(gamma=0.0, alpha=None)


class WeightedSoftmaxClassificationLoss:
    """losses.py:356-391 (one-hot targets)"""

    def __init__(self, logit_scale=1.0):
        self._logit_scale = logit_scale

    def __call__(self, prediction_tensor, target_tensor, weights):
        C = prediction_tensor.shape[-1]
        ce = F.cross_entropy((prediction_tensor / self._logit_scale).reshape(-1, C), target_tensor.reshape(-1, C).argmax(-1), reduction="none")
        return ce.reshape(weights.shape) * weights


# ---- the reference's five functions (detectors/pointpillars.py:468-585), names and argument lists kept -----------------------------------

def prepare_loss_weights(labels, pos_cls_weight=1.0, neg_cls_weight=1.0, loss_norm_type="NormByNumPositives", dtype=torch.float32):
    """pointpillars.py:468-506.  cls_weights carries neg_cls_weight on EVERY anchor, the don't-care ones included (:480)."""
    cared = labels >= 0
    positives, negatives = labels > 0, labels == 0
    cls_weights = neg_cls_weight + pos_cls_weight * positives.to(dtype)
    reg_weights = positives.to(dtype)
    if loss_norm_type == "NormByNumExamples":
        cls_weights = cls_weights / torch.clamp(cared.to(dtype).sum(1, keepdim=True), min=1.0)
        reg_weights = reg_weights / torch.clamp(positives.sum(1, keepdim=True).to(dtype), min=1.0)
    elif loss_norm_type == "NormByNumPositives":
        pos_normalizer = torch.clamp(positives.to(dtype).sum(1, keepdim=True), min=1.0)
        reg_weights = reg_weights / pos_normalizer
        cls_weights = cls_weights / pos_normalizer
    elif loss_norm_type == "NormByNumPosNeg":
        pos_neg = torch.stack([positives, negatives], dim=-1).to(dtype)
        normalizer = pos_neg.sum(1, keepdim=True)                          # [N, 1, 2]
        cls_normalizer = torch.clamp((pos_neg * normalizer).sum(-1), min=1.0)
        normalizer = torch.clamp(normalizer, min=1.0)
        reg_weights = reg_weights / normalizer[:, 0:1, 0]
        cls_weights = cls_weights / cls_normalizer
    else:
        raise ValueError("unknown loss norm type.")
    return cls_weights, reg_weights, cared


def add_sin_difference(boxes1, boxes2):
    """pointpillars.py:551-557"""
    rad_pred_encoding = torch.sin(boxes1[:, :, -1:]) * torch.cos(boxes2[:, :, -1:])
    rad_tg_encoding = torch.cos(boxes1[:, :, -1:]) * torch.sin(boxes2[:, :, -1:])
    return torch.cat([boxes1[:, :, :-1], rad_pred_encoding], dim=-1), torch.cat([boxes2[:, :, :-1], rad_tg_encoding], dim=-1)


def create_loss(loc_loss_ftor, cls_loss_ftor, box_preds, cls_preds, cls_targets, cls_weights, reg_targets, reg_weights, num_class,
                encode_background_as_zeros=True, encode_rad_error_by_sin=True, box_code_size=7):
    """pointpillars.py:508-549"""
    batch_size = int(box_preds.shape[0])
    box_preds = box_preds.reshape(batch_size, -1, box_code_size)
    cls_preds = cls_preds.reshape(batch_size, -1, num_class if encode_background_as_zeros else num_class + 1)
    cls_targets = cls_targets.squeeze(-1)
    classes = torch.arange(num_class + 1, device=cls_targets.device, dtype=cls_targets.dtype)
    one_hot_targets = (cls_targets.unsqueeze(-1) == classes).to(box_preds.dtype)
    if encode_background_as_zeros:
        one_hot_targets = one_hot_targets[:, :, 1:]
    if encode_rad_error_by_sin:
        box_preds, reg_targets = add_sin_difference(box_preds, reg_targets)
    loc_losses = loc_loss_ftor(box_preds, reg_targets, weights=reg_weights)
    cls_losses = cls_loss_ftor(cls_preds, one_hot_targets, weights=cls_weights)
    return loc_losses, cls_losses


def _get_pos_neg_loss(cls_loss, labels):
    """pointpillars.py:559-573"""
    batch_size = cls_loss.shape[0]
    if cls_loss.shape[-1] == 1 or cls_loss.dim() == 2:
        cls_pos_loss = ((labels > 0).to(cls_loss.dtype) * cls_loss.reshape(batch_size, -1)).sum() / batch_size
        cls_neg_loss = ((labels == 0).to(cls_loss.dtype) * cls_loss.reshape(batch_size, -1)).sum() / batch_size
    else:
        cls_pos_loss = cls_loss[:, :, 1:].sum() / batch_size
        cls_neg_loss = cls_loss[:, :, 0].sum() / batch_size
    return cls_pos_loss, cls_neg_loss


def get_direction_target(anchors, reg_targets, one_hot=True):
    """pointpillars.py:575-585"""
    batch_size = reg_targets.shape[0]
    anchors = anchors.reshape(batch_size, -1, 7)
    rot_gt = reg_targets[:, :, -1] + anchors[:, :, -1]
    dir_cls_targets = (rot_gt > 0).to(torch.int64)
    if one_hot:
        dir_cls_targets = F.one_hot(dir_cls_targets, 2).to(anchors.dtype)
    return dir_cls_targets


# ---- the node ----------------------------------------------------------------------------------------------------------------------------

class _DetLoss(torch.autograd.Function):
    """(box_preds [B,A,k], cls_preds [B,A,C'], dir_preds [B,A,2] | None, labels [B,A], reg_targets, anchors | None) ->
    (loss, reduced [5], cls_loss | None, loc_loss | None, cared); only ``loss`` is differentiable."""

    @staticmethod
    def forward(ctx, hp, box, cls, dirp, labels, tgt, anchors):
        lib, dev = _lib.load(), box.device
        B, A = labels.shape
        d = DetLossDesc()
        d.B, d.A, d.code_size = B, A, box.shape[-1]
        d.C = cls.shape[-1] if hp["encode_background_as_zeros"] else cls.shape[-1] - 1
        d.norm_type = NORM_TYPES[hp["loss_norm_type"]]
        d.has_alpha, d.alpha = (0, 0.0) if hp["alpha"] is None else (1, float(hp["alpha"]))
        d.sin_diff, d.has_dir = int(bool(hp["encode_rad_error_by_sin"])), int(dirp is not None)
        d.encode_background_as_zeros, d.codewise = int(bool(hp["encode_background_as_zeros"])), int(bool(hp["codewise"]))
        d.labels_i64 = int(labels.dtype == torch.int64)
        d.pos_cls_weight, d.neg_cls_weight = float(hp["pos_cls_weight"]), float(hp["neg_cls_weight"])
        d.gamma, d.sigma = float(hp["gamma"]), float(hp["sigma"])
        cw = hp["code_weights"]
        if cw is not None and len(cw) != 7:
            raise _lib.PapcError("pointpillars_loss: %d code weights (the kernels are built for a box code size of 7)" % len(cw))
        d.code_weights = (c_f * 7)(*([1.0] * 7 if cw is None else [float(v) for v in cw]))
        d.loc_weight, d.cls_weight, d.dir_weight = float(hp["loc_weight"]), float(hp["cls_weight"]), float(hp["direction_loss_weight"])
        nbytes = ctypes.c_int64(0)
        check(lib.papc_det_loss_workspace(ctypes.byref(d), ctypes.byref(nbytes)), "papc_det_loss_workspace")    # refuses what is not built

        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)      # noqa: E731
        n = B * A
        grads = new(n * (2 * d.has_dir + 7 + d.C))          # [ddir | dbox | dcls]: one buffer, one scaling launch in the backward
        o_dir, o_box = 2 * d.has_dir * n, (2 * d.has_dir + 7) * n
        out = new(8)
        ws = torch.empty(nbytes.value, device=dev, dtype=torch.uint8)
        cls_loss = new(B, A, d.C) if hp["per_anchor_losses"] else None
        loc_loss = new(B, A, 7) if hp["per_anchor_losses"] else None
        cared = torch.empty(B, A, device=dev, dtype=torch.bool)
        io = DetLossIo()
        io.box_preds, io.cls_preds, io.dir_preds, io.labels, io.reg_targets, io.anchors = ptr(box), ptr(cls), ptr(dirp), ptr(labels), ptr(tgt), ptr(anchors)
        io.out, io.ddir, io.dbox, io.dcls = ptr(out), ptr(grads) if d.has_dir else None, ptr(grads) + 4 * o_dir, ptr(grads) + 4 * o_box
        io.cls_loss, io.loc_loss, io.cared, io.workspace = ptr(cls_loss), ptr(loc_loss), ptr(cared), ptr(ws)
        check(lib.papc_det_loss_fwd_f32(ctypes.byref(d), ctypes.byref(io), stream_ptr()), "papc_det_loss_fwd_f32")
        ctx.save_for_backward(grads)
        ctx.split = (o_dir, o_box, box.shape, cls.shape, None if dirp is None else dirp.shape)
        loss, reduced = out[0], out[1:6]
        ctx.mark_non_differentiable(*[t for t in (reduced, cls_loss, loc_loss, cared) if t is not None])
        ctx.set_materialize_grads(False)          # no zero-filled gradient tensors for the by-products: four launches of a backward
        return loss, reduced, cls_loss, loc_loss, cared

    @staticmethod
    def backward(ctx, g, *_):
        from .head import _scale_dz
        if g is None:
            return (None,) * 7
        (grads,) = ctx.saved_tensors
        o_dir, o_box, sbox, scls, sdir = ctx.split
        grads = _scale_dz(grads, g)
        return (None, grads[o_dir:o_box].view(sbox), grads[o_box:].view(scls), None if sdir is None else grads[:o_dir].view(sdir),
                None, None, None)


def _hyper(num_class, pos_cls_weight, neg_cls_weight, loss_norm_type, alpha, gamma, sigma, code_weights, codewise, encode_rad_error_by_sin,
           encode_background_as_zeros, box_code_size, use_direction_classifier, loc_weight, cls_weight, direction_loss_weight,
           per_anchor_losses):
    if loss_norm_type not in NORM_TYPES:
        raise ValueError("unknown loss norm type.")
    return dict(locals())


def _shape_inputs(hp, box_preds, cls_preds, dir_cls_preds, labels, reg_targets, anchors):
    """the RPN's [B, H, W, n * k] maps (or [B, A, k] already) -> [B, A, k]"""
    B = int(box_preds.shape[0])
    box = box_preds.reshape(B, -1, hp["box_code_size"])
    cls = cls_preds.reshape(B, -1, hp["num_class"] if hp["encode_background_as_zeros"] else hp["num_class"] + 1)
    use_dir = hp["use_direction_classifier"] and dir_cls_preds is not None
    dirp = dir_cls_preds.reshape(B, -1, 2) if use_dir else None
    A = box.shape[1]
    labels = labels.reshape(B, A)
    reg_targets = reg_targets.reshape(B, A, hp["box_code_size"])
    anchors = anchors.reshape(B, A, -1) if use_dir else None
    if cls.shape[1] != A or (dirp is not None and dirp.shape[1] != A):
        raise ValueError("pointpillars_loss: box_preds give %d anchors, cls_preds %d%s" % (A, cls.shape[1], "" if dirp is None else ", dir_cls_preds %d" % dirp.shape[1]))
    return box, cls, dirp, labels, reg_targets, anchors


def _loss_torch(hp, box, cls, dirp, labels, reg_targets, anchors, cls_preds):
    B, dtype = box.shape[0], box.dtype
    cls_weights, reg_weights, cared = prepare_loss_weights(labels, hp["pos_cls_weight"], hp["neg_cls_weight"], hp["loss_norm_type"], dtype)
    cls_targets = (labels * cared.to(labels.dtype)).unsqueeze(-1)
    loc_ftor = WeightedSmoothL1LocalizationLoss(hp["sigma"], hp["code_weights"], hp["codewise"])
    cls_ftor = SigmoidFocalClassificationLoss(hp["gamma"], hp["alpha"])
    loc_loss, cls_loss = create_loss(loc_ftor, cls_ftor, box, cls, cls_targets, cls_weights, reg_targets, reg_weights, hp["num_class"],
                                     hp["encode_background_as_zeros"], hp["encode_rad_error_by_sin"], hp["box_code_size"])
    loc_loss_reduced = loc_loss.sum() / B * hp["loc_weight"]
    cls_pos_loss, cls_neg_loss = _get_pos_neg_loss(cls_loss, labels)
    cls_loss_reduced = cls_loss.sum() / B * hp["cls_weight"]
    loss = loc_loss_reduced + cls_loss_reduced
    dir_loss = torch.zeros((), device=box.device, dtype=dtype)
    if dirp is not None:
        dir_targets = get_direction_target(anchors, reg_targets)
        weights = (labels > 0).to(dtype)
        weights = weights / torch.clamp(weights.sum(-1, keepdim=True), min=1.0)
        dir_loss = WeightedSoftmaxClassificationLoss()(dirp, dir_targets, weights=weights).sum() / B
        loss = loss + dir_loss * hp["direction_loss_weight"]
    return {"loss": loss, "cls_loss": cls_loss, "loc_loss": loc_loss, "cls_pos_loss": cls_pos_loss / hp["pos_cls_weight"],
            "cls_neg_loss": cls_neg_loss / hp["neg_cls_weight"], "cls_preds": cls_preds, "dir_loss_reduced": dir_loss,
            "cls_loss_reduced": cls_loss_reduced, "loc_loss_reduced": loc_loss_reduced, "cared": cared}


# the keyword defaults: params/configs/pointpillars_kitti_car_xy16.yaml (LOSS, BACKBONE, ENCODE_RAD_ERROR_BY_SIN, NUM_CLASS)
def pointpillars_loss(box_preds, cls_preds, dir_cls_preds, labels, reg_targets, anchors, *, num_class=2, pos_cls_weight=1.0,
                      neg_cls_weight=1.0, loss_norm_type="NormByNumPositives", alpha=0.25, gamma=2.0, sigma=3.0,
                      code_weights=(1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0), codewise=True, encode_rad_error_by_sin=False,
                      encode_background_as_zeros=True, box_code_size=7, use_direction_classifier=True, loc_weight=2.0, cls_weight=1.0,
                      direction_loss_weight=2.0, per_anchor_losses=True, fused=None):
    """The training branch of PointPillars.forward (pointpillars.py:150-213) -> the reference's result dict: loss, cls_loss [B,A,C], loc_loss
    [B,A,7], cls_pos_loss, cls_neg_loss, cls_preds (the argument), dir_loss_reduced, cls_loss_reduced, loc_loss_reduced, cared [B,A] bool.

    box_preds [B,H,W,n*7] (or [B,A,7]), cls_preds [B,H,W,n*C], dir_cls_preds [B,H,W,n*2] or None, labels [B,A] int64 / int32 (< 0 don't
    care, 0 negative, k > 0 class k), reg_targets [B,A,7], anchors [B,A,7].  The keyword defaults are the KITTI car yaml's; ``alpha=None``
    with ``gamma=0`` is the weighted sigmoid loss.  Only ``loss`` carries a gradient on the fused node (the dict's other entries are for
    logging); ``per_anchor_losses=False`` leaves cls_loss / loc_loss out (None) and saves their stores.  Arguments the kernels are not
    built for (C > 8, a code size other than 7, encode_background_as_zeros=False, codewise=False) raise PapcError; PAPC_DET_LOSS=0
    computes them in torch ops.  ``fused``: None = as PAPC_DET_LOSS says, False = the torch-op flavour, True = the node."""
    hp = _hyper(num_class, pos_cls_weight, neg_cls_weight, loss_norm_type, alpha, gamma, sigma, code_weights, codewise,
                encode_rad_error_by_sin, encode_background_as_zeros, box_code_size, use_direction_classifier, loc_weight, cls_weight,
                direction_loss_weight, per_anchor_losses)
    box, cls, dirp, lab, tgt, anc = _shape_inputs(hp, box_preds, cls_preds, dir_cls_preds, labels, reg_targets, anchors)
    if not (fused_enabled() if fused is None else fused):
        return _loss_torch(hp, box, cls, dirp, lab, tgt, anc, cls_preds)
    if not box.is_cuda:
        raise _lib.PapcError("pointpillars_loss needs CUDA (ROCm) tensors: there is no CPU fallback (PAPC_DET_LOSS=0 selects the torch-op flavour)")
    f32 = lambda t: None if t is None else t.contiguous().float()      # noqa: E731
    if lab.dtype not in (torch.int32, torch.int64):
        lab = lab.to(torch.int64)
    loss, red, cls_loss, loc_loss, cared = _DetLoss.apply(hp, f32(box), f32(cls), f32(dirp), lab.contiguous(), f32(tgt), f32(anc))
    return {"loss": loss, "cls_loss": cls_loss, "loc_loss": loc_loss, "cls_pos_loss": red[3], "cls_neg_loss": red[4], "cls_preds": cls_preds,
            "dir_loss_reduced": red[2], "cls_loss_reduced": red[1], "loc_loss_reduced": red[0], "cared": cared}
