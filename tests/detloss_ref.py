"""float64 restatement of the PointPillars detection loss for the tests, torch on the CPU, differentiable: the five functions of
PAPC/models/detect/pointpillars/models/detectors/pointpillars.py (prepare_loss_weights :468-506, create_loss :508-549, add_sin_difference
:551-557, _get_pos_neg_loss :559-573, get_direction_target :575-585), the three loss classes of core/losses.py the detector uses (smooth L1
:134-183, sigmoid focal :234-292 -- with gamma = 0 and no alpha the weighted sigmoid loss :202-231 --, weighted softmax :356-391) and the
training branch of PointPillars.forward (:150-213) that strings them together.  The op sequence is the source's, line by line.

One deliberate float32 step: the direction target is taken from the FLOAT32 sum reg_targets[..., 6] + anchors[..., 6] (:579) -- the threshold
at zero is discontinuous, and float32 is what the reference and both flavours under test add in.
"""
import torch
import torch.nn.functional as F

F64 = torch.float64


def prepare_loss_weights(labels, pos_cls_weight=1.0, neg_cls_weight=1.0, loss_norm_type="NormByNumPositives", dtype=F64):
    cared = labels >= 0                                                                  # :475
    positives = labels > 0
    negatives = labels == 0
    cls_weights = neg_cls_weight + pos_cls_weight * positives.to(dtype)                  # :480: every anchor, don't-care ones included
    reg_weights = positives.to(dtype)
    if loss_norm_type == "NormByNumExamples":                                            # :483-488
        num_examples = torch.clamp(cared.to(dtype).sum(1, keepdim=True), min=1.0)
        cls_weights = cls_weights / num_examples
        bbox_normalizer = positives.sum(1, keepdim=True).to(dtype)
        reg_weights = reg_weights / torch.clamp(bbox_normalizer, min=1.0)
    elif loss_norm_type == "NormByNumPositives":                                         # :489-492
        pos_normalizer = positives.to(dtype).sum(1, keepdim=True)
        reg_weights = reg_weights / torch.clamp(pos_normalizer, min=1.0)
        cls_weights = cls_weights / torch.clamp(pos_normalizer, min=1.0)
    elif loss_norm_type == "NormByNumPosNeg":                                            # :493-501
        pos_neg = torch.stack([positives, negatives], dim=-1).to(dtype)
        normalizer = pos_neg.sum(1, keepdim=True)
        cls_normalizer = (pos_neg * normalizer).sum(-1)
        cls_normalizer = torch.clamp(cls_normalizer, min=1.0)
        normalizer = torch.clamp(normalizer, min=1.0)
        reg_weights = reg_weights / normalizer[:, 0:1, 0]
        cls_weights = cls_weights / cls_normalizer
    else:
        raise ValueError("unknown loss norm type.")
    return cls_weights, reg_weights, cared


def smooth_l1(prediction, target, weights, sigma=3.0, code_weights=None):
    """WeightedSmoothL1LocalizationLoss._compute_loss, codewise (losses.py:166-177)"""
    diff = prediction - target
    if code_weights is not None:
        diff = torch.as_tensor(code_weights, dtype=F64).reshape(1, 1, -1) * diff
    abs_diff = torch.abs(diff)
    lt = (abs_diff <= 1 / (sigma ** 2)).to(F64)
    loss = lt * 0.5 * torch.pow(abs_diff * sigma, 2) + (abs_diff - 0.5 / (sigma ** 2)) * (1.0 - lt)
    return loss * weights.unsqueeze(-1)


def sigmoid_cross_entropy(logits, labels):
    """losses.py:185-189"""
    loss = torch.clamp(logits, min=0) - logits * labels
    return loss + torch.log1p(torch.exp(-torch.abs(logits)))


def sigmoid_focal(prediction, target, weights, gamma=2.0, alpha=0.25):
    """SigmoidFocalClassificationLoss._compute_loss (losses.py:273-292); gamma = 0, alpha = None: WeightedSigmoidClassificationLoss (:225-231)"""
    per_entry_cross_ent = sigmoid_cross_entropy(prediction, target)
    prediction_probabilities = torch.sigmoid(prediction)
    p_t = target * prediction_probabilities + (1 - target) * (1 - prediction_probabilities)
    modulating_factor = 1.0
    if gamma:
        modulating_factor = torch.pow(1.0 - p_t, gamma)
    alpha_weight_factor = 1.0
    if alpha is not None:
        alpha_weight_factor = target * alpha + (1 - target) * (1 - alpha)
    return modulating_factor * alpha_weight_factor * per_entry_cross_ent * weights.unsqueeze(2)


def weighted_softmax(prediction, target_one_hot, weights):
    """WeightedSoftmaxClassificationLoss._compute_loss at logit_scale 1 (losses.py:385-391)"""
    C = prediction.shape[-1]
    ce = F.cross_entropy(prediction.reshape(-1, C), target_one_hot.reshape(-1, C).argmax(-1), reduction="none")
    return ce.reshape(weights.shape) * weights


def add_sin_difference(boxes1, boxes2):
    rad_pred_encoding = torch.sin(boxes1[:, :, -1:]) * torch.cos(boxes2[:, :, -1:])      # :552-554
    rad_tg_encoding = torch.cos(boxes1[:, :, -1:]) * torch.sin(boxes2[:, :, -1:])
    return torch.cat([boxes1[:, :, :-1], rad_pred_encoding], -1), torch.cat([boxes2[:, :, :-1], rad_tg_encoding], -1)


def create_loss(box_preds, cls_preds, cls_targets, cls_weights, reg_targets, reg_weights, num_class, gamma, alpha, sigma, code_weights,
                encode_rad_error_by_sin=True):
    """:508-549 with encode_background_as_zeros = True and a box code size of 7"""
    B = box_preds.shape[0]
    box_preds = box_preds.reshape(B, -1, 7)
    cls_preds = cls_preds.reshape(B, -1, num_class)
    one_hot_targets = F.one_hot(cls_targets.squeeze(-1), num_class + 1).to(F64)[:, :, 1:]    # :528-534
    if encode_rad_error_by_sin:
        box_preds, reg_targets = add_sin_difference(box_preds, reg_targets)
    loc_losses = smooth_l1(box_preds, reg_targets, reg_weights, sigma, code_weights)
    cls_losses = sigmoid_focal(cls_preds, one_hot_targets, cls_weights, gamma, alpha)
    return loc_losses, cls_losses


def get_pos_neg_loss(cls_loss, labels):
    B = cls_loss.shape[0]                                                                # :563-571
    if cls_loss.shape[-1] == 1 or cls_loss.dim() == 2:
        cls_pos_loss = ((labels > 0).to(F64) * cls_loss.reshape(B, -1)).sum() / B
        cls_neg_loss = ((labels == 0).to(F64) * cls_loss.reshape(B, -1)).sum() / B
    else:
        cls_pos_loss = cls_loss[:, :, 1:].sum() / B
        cls_neg_loss = cls_loss[:, :, 0].sum() / B
    return cls_pos_loss, cls_neg_loss


def get_direction_target(anchors, reg_targets):
    """:575-585; anchors / reg_targets FLOAT32: the sum is taken in float32 (see the module docstring) -> (class index int64, one-hot float64)"""
    B = reg_targets.shape[0]
    rot_gt = reg_targets.float()[:, :, -1] + anchors.float().reshape(B, -1, 7)[:, :, -1]
    idx = (rot_gt > 0).to(torch.int64)
    return idx, F.one_hot(idx, 2).to(F64)


def pointpillars_loss(box_preds, cls_preds, dir_cls_preds, labels, reg_targets, anchors, *, num_class=1, pos_cls_weight=1.0,
                      neg_cls_weight=1.0, loss_norm_type="NormByNumPositives", alpha=0.25, gamma=2.0, sigma=3.0, code_weights=None,
                      encode_rad_error_by_sin=False, loc_weight=2.0, cls_weight=1.0, direction_loss_weight=2.0):
    """PointPillars.forward's training branch (:150-213).  box_preds / cls_preds / dir_cls_preds: float64 leaves (dir_cls_preds None: no
    direction term); labels int64 [B, A]; reg_targets, anchors: the FLOAT32 tensors the flavours under test get.  -> the result dict plus
    ``dir_targets`` (int64 [B, A])."""
    B = box_preds.shape[0]
    labels = labels.long()
    tgt64 = reg_targets.to(F64)
    cls_weights, reg_weights, cared = prepare_loss_weights(labels, pos_cls_weight, neg_cls_weight, loss_norm_type)
    cls_targets = (labels * cared.to(labels.dtype)).unsqueeze(-1)                        # :161-162
    loc_loss, cls_loss = create_loss(box_preds, cls_preds, cls_targets, cls_weights, tgt64, reg_weights, num_class, gamma, alpha, sigma,
                                     code_weights, encode_rad_error_by_sin)
    loc_loss_reduced = loc_loss.sum() / B * loc_weight                                   # :181-182
    cls_pos_loss, cls_neg_loss = get_pos_neg_loss(cls_loss, labels)
    cls_pos_loss = cls_pos_loss / pos_cls_weight
    cls_neg_loss = cls_neg_loss / neg_cls_weight
    cls_loss_reduced = cls_loss.sum() / B * cls_weight                                   # :186-187
    loss = loc_loss_reduced + cls_loss_reduced
    dir_loss, dir_idx = torch.zeros((), dtype=F64), None
    if dir_cls_preds is not None:                                                        # :190-199
        dir_idx, dir_targets = get_direction_target(anchors, reg_targets)
        dir_logits = dir_cls_preds.reshape(B, -1, 2)
        weights = (labels > 0).to(F64)
        weights = weights / torch.clamp(weights.sum(-1, keepdim=True), min=1.0)
        dir_loss = weighted_softmax(dir_logits, dir_targets, weights).sum() / B
        loss = loss + dir_loss * direction_loss_weight
    return {"loss": loss, "cls_loss": cls_loss, "loc_loss": loc_loss, "cls_pos_loss": cls_pos_loss, "cls_neg_loss": cls_neg_loss,
            "cls_preds": cls_preds, "dir_loss_reduced": dir_loss, "cls_loss_reduced": cls_loss_reduced, "loc_loss_reduced": loc_loss_reduced,
            "cared": cared, "dir_targets": dir_idx}
