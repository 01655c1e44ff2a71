"""The PointPillars detector as thin glue over this package's stages: PillarFeatureNet -> PointPillarsScatter -> RPN, then the detection loss
(train mode) or predict() (eval mode).

Reference: PAPC/models/detect/pointpillars/models/detectors/pointpillars.py:27-216.  The reference builds itself from its config system; here
the same choices are plain keyword arguments (DESIGN 7 keeps the config system out).  No kernels of its own.
"""
import torch.nn as nn

from . import detect, detloss
from .pillars import PillarFeatureNet
from .rpn import RPN
from .voxel import PointPillarsScatter


class PointPillars(nn.Module):
    """forward(example) with the keys of pointpillars.py:125-213: "voxels" [P, T, F], "num_points" [P], "coordinates" [P, 4] = (batch, z, y, x),
    "anchors" [B, A, 7]; train mode adds "labels" [B, A] and "reg_targets" [B, A, 7] and returns detloss.pointpillars_loss's dict; eval mode
    takes "image_idx" [B] (and "anchors_mask") and returns detect.predict's list of per-frame dicts.

    ``output_shape`` = [_, _, ny, nx] of the canvas, ``pfn`` / ``rpn`` the keyword arguments of PillarFeatureNet / RPN (num_class, the input
    filters and the code size are filled in from the other arguments), ``loss`` those of detloss.pointpillars_loss and ``post`` those of
    detect.predict (the four nms_* values are required there)."""

    def __init__(self, output_shape, num_class=1, num_anchor_per_loc=2, box_code_size=7, encode_background_as_zeros=True,
                 use_direction_classifier=True, pfn=None, rpn=None, loss=None, post=None):
        super().__init__()
        pfn, rpn = dict(pfn or {}), dict(rpn or {})
        pfn.setdefault("num_filters", (64,))
        self.pfn = PillarFeatureNet(**pfn)                                                     # :74-79
        self.mfe = PointPillarsScatter(output_shape=output_shape, num_input_features=pfn["num_filters"][-1])      # :82-83
        rpn.update(num_class=num_class, num_input_filters=self.mfe.nchannels, num_anchor_per_loc=num_anchor_per_loc,
                   encode_background_as_zeros=encode_background_as_zeros, use_direction_classifier=use_direction_classifier,
                   box_code_size=box_code_size)
        self.rpn = RPN(**rpn)                                                                  # :86-102
        common = dict(num_class=num_class, encode_background_as_zeros=encode_background_as_zeros, use_direction_classifier=use_direction_classifier)
        self._loss_kw = dict(loss or {}, box_code_size=box_code_size, **common)
        self._post_kw = dict(post or {}, **common)

    def forward(self, example):
        anchors = example["anchors"]
        batch_size = int(anchors.shape[0])                                                     # :131
        voxel_features = self.pfn(example["voxels"], example["num_points"], example["coordinates"])               # :137
        spatial_features = self.mfe(voxel_features, example["coordinates"], batch_size)        # :139
        preds = self.rpn(spatial_features)                                                     # :144
        if self.training:                                                                      # :149-213
            return detloss.pointpillars_loss(preds["box_preds"], preds["cls_preds"], preds.get("dir_cls_preds"), example["labels"],
                                             example["reg_targets"], anchors.reshape(batch_size, -1, anchors.shape[-1]), **self._loss_kw)
        return detect.predict(example, preds, **self._post_kw)                                 # :216
