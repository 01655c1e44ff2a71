"""PointPillars training targets on the device: anchors, the occupied-area anchor mask and ``TargetAssigner.assign`` (csrc/dettarget.hip).

Mirrors the host pipeline of data/preprocess.py:251-302: anchor generation (core/anchor_generator.py, core/target_assigner.py:58-85,
libs/ops/box_np_ops.py:519-595), the anchor mask (box_np_ops.py:772-805), ``create_target_np`` (libs/ops/target_ops.py:31-214) on
``NearestIouSimilarity`` (core/similarity_calculator.py:73-93, box_np_ops.py:244-256, :654-682) and ``second_box_encode`` (box_np_ops.py:30-66).
What is static -- the anchors, their near-bboxes, their cell boxes in the pillar grid, the thresholds -- is computed ONCE on the host by
``anchor_cache``; what changes per frame runs on the device: ``anchors_mask`` from the voxeliser's ``coors`` and ``assign`` from a padded batch of
ground-truth boxes, each one launch sequence for the batch with no host synchronisation.  ``assign``'s ``labels`` / ``reg_targets`` are what
``detloss.pointpillars_loss`` takes, ``anchors_mask``'s bytes what ``detect.predict_tensors`` takes.

Kept as the source has them:
  * the mask's four-corner expression S[y2,x2] - S[y2,x1] - S[y1,x2] + S[y1,x1] leaves out the min cell's row and column;
  * ``generate_anchors`` concatenates the anchors of several generators on axis -2 but their threshold vectors on axis 0, so with generators of
    different thresholds the vectors do not follow the anchors' order;
  * a force-matched anchor takes the class and the box of its OWN argmax gt, not of the gt that forced it;
  * labels are written matched, then background, then forced again: with unmatched > matched an anchor in between is background.
Where the source does not run as written, the intent is taken: ``np.meshgrid`` returns a tuple under current numpy and the source assigns into it.

Not built: ``positive_fraction`` (the source samples with numpy's global RNG; no parity can be stated) -- ``assign`` raises for it.  At most 256
ground-truth rows per frame (``Gmax``).

``PAPC_DET_TARGETS=0`` (environment, read once at import, as PAPC_DET_LOSS / PAPC_DET_POST are) runs the second flavour: the same semantics in
vectorised float32 torch ops in the same operation order, frame by frame, with host synchronisation.  It is the A/B leg and runs on CPU tensors too.
"""
import ctypes

import numpy as np
import torch

from . import _lib, boxcodec
from .boxcodec import _const, _encode_torch
from ._lib import c_p, c_f, check, ptr, stream_ptr


class AnchorsMaskDesc(ctypes.Structure):
    """papc_anchors_mask_desc"""
    _fields_ = [("B", ctypes.c_int32), ("A", ctypes.c_int32), ("ny", ctypes.c_int32), ("nx", ctypes.c_int32), ("P", ctypes.c_int64),
                ("area_thresh", c_f), ("reserved", ctypes.c_int32)]


class AnchorsMaskIo(ctypes.Structure):
    """papc_anchors_mask_io"""
    _fields_ = [("coors", c_p), ("cells", c_p), ("mask", c_p)]


class DetAssignDesc(ctypes.Structure):
    """papc_det_assign_desc"""
    _fields_ = [("B", ctypes.c_int32), ("A", ctypes.c_int32), ("Gmax", ctypes.c_int32), ("encode_angle_to_vector", ctypes.c_int32),
                ("smooth_dim", ctypes.c_int32), ("code_size", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("reserved1", ctypes.c_int32)]


class DetAssignIo(ctypes.Structure):
    """papc_det_assign_io"""
    _fields_ = [("anchors", c_p), ("anchors_bv", c_p), ("matched", c_p), ("unmatched", c_p), ("anchors_mask", c_p), ("gt_boxes", c_p),
                ("gt_classes", c_p), ("num_gt", c_p), ("labels", c_p), ("reg_targets", c_p), ("reg_weights", c_p), ("gt_ids", c_p),
                ("max_overlap", c_p), ("num_pos", c_p)]


_DET_TARGETS = _lib.env_switch("PAPC_DET_TARGETS")               # A/B switch: 0 = the torch-op flavour

GMAX_LIMIT = 256


def fused_enabled():
    """what PAPC_DET_TARGETS selected"""
    return _DET_TARGETS


def _use_fused(fused):
    return fused_enabled() if fused is None else bool(fused)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# anchors (host, once)

def _anchor_grid(z_centers, y_centers, x_centers, sizes, rotations, dtype):
    """[D,H,W,num_sizes,num_rots,7] = (x, y, z, size..., rotation): the layout box_np_ops.py:544-557 builds by meshgrid / tile / transpose"""
    sizes = np.array(sizes, dtype=dtype).reshape(-1, 3)
    rotations = np.array(rotations, dtype=dtype)
    out = np.empty((len(z_centers), len(y_centers), len(x_centers), sizes.shape[0], len(rotations), 7), dtype=dtype)
    out[..., 0] = x_centers[None, None, :, None, None]
    out[..., 1] = y_centers[None, :, None, None, None]
    out[..., 2] = z_centers[:, None, None, None, None]
    out[..., 3:6] = sizes[None, None, None, :, None, :]
    out[..., 6] = rotations[None, None, None, None, :]
    return out


class _AnchorGenerator:
    def __init__(self, sizes, rotations, class_id, match_threshold, unmatch_threshold, dtype):
        self._sizes, self._rotations, self._dtype = sizes, rotations, dtype
        self._class_id, self._match_threshold, self._unmatch_threshold = class_id, match_threshold, unmatch_threshold

    @property
    def class_id(self):
        return self._class_id

    @property
    def match_threshold(self):
        return self._match_threshold

    @property
    def unmatch_threshold(self):
        return self._unmatch_threshold

    @property
    def num_anchors_per_localization(self):
        return len(self._rotations) * np.array(self._sizes).reshape(-1, 3).shape[0]


class AnchorGeneratorStride(_AnchorGenerator):
    """core/anchor_generator.py:5-45 on create_anchors_3d_stride (box_np_ops.py:519-557): centres arange(n) * stride + offset, in ``dtype``"""

    def __init__(self, sizes=(1.6, 3.9, 1.56), anchor_strides=(0.4, 0.4, 1.0), anchor_offsets=(0.2, -39.8, -1.78), rotations=(0, np.pi / 2),
                 class_id=None, match_threshold=-1, unmatch_threshold=-1, dtype=np.float32):
        super().__init__(sizes, rotations, class_id, match_threshold, unmatch_threshold, dtype)
        self._anchor_strides, self._anchor_offsets = anchor_strides, anchor_offsets

    def generate(self, feature_map_size):
        """feature_map_size (D, H, W) -> [D,H,W,num_sizes,num_rots,7]"""
        centers = []
        for n, stride, offset in zip(feature_map_size, self._anchor_strides[::-1], self._anchor_offsets[::-1]):      # z, y, x
            centers.append(np.arange(n, dtype=self._dtype) * stride + offset)
        return _anchor_grid(centers[0], centers[1], centers[2], self._sizes, self._rotations, self._dtype)


class AnchorGeneratorRange(_AnchorGenerator):
    """core/anchor_generator.py:47-85 on create_anchors_3d_range (box_np_ops.py:560-595): centres linspace(lo, hi, n) of the range cast to ``dtype``"""

    def __init__(self, anchor_ranges, sizes=(1.6, 3.9, 1.56), rotations=(0, np.pi / 2), class_id=None, match_threshold=-1, unmatch_threshold=-1,
                 dtype=np.float32):
        super().__init__(sizes, rotations, class_id, match_threshold, unmatch_threshold, dtype)
        self._anchor_ranges = anchor_ranges

    def generate(self, feature_map_size):
        r = np.array(self._anchor_ranges, self._dtype)
        z, y, x = (np.linspace(r[2 - k], r[5 - k], feature_map_size[k], dtype=self._dtype) for k in range(3))
        return _anchor_grid(z, y, x, self._sizes, self._rotations, self._dtype)


def rbbox2d_to_near_bbox(rbboxes):
    """box_np_ops.py:244-256 in the tensor's dtype: [N,5] (x, y, xdim, ydim, rad) -> [N,4] (xmin, ymin, xmax, ymax) of the nearest axis-aligned box"""
    rots = rbboxes[..., 4]
    pi = _const(np.pi, rbboxes)
    lim = rots - torch.floor(rots / pi + _const(0.5, rbboxes)) * pi                  # limit_period(rots, 0.5, np.pi)
    cond = (torch.abs(lim) > _const(np.pi / 4, rbboxes))[..., None]
    dims = torch.where(cond, rbboxes[..., [3, 2]], rbboxes[..., 2:4])
    half = dims / _const(2.0, rbboxes)
    return torch.cat([rbboxes[..., :2] - half, rbboxes[..., :2] + half], dim=-1)


def anchor_cells(anchors_bv, voxel_size, point_cloud_range, grid_size):
    """The cell box (x1, y1, x2, y2) of every anchor in the pillar grid, int32 [A,4]: floor((bv - offset) / stride) in float32, min corner held to
    >= 0 and max corner to <= grid - 1 (box_np_ops.py:788-799).  Raises if a cell is outside the grid after those one-sided clamps (the source
    would index from the map's far end, or past it)."""
    bv = np.asarray(anchors_bv, dtype=np.float32)
    stride, offset = np.asarray(voxel_size, dtype=np.float32), np.asarray(point_cloud_range, dtype=np.float32)
    nx, ny = int(grid_size[0]), int(grid_size[1])
    cells = np.empty(bv.shape, dtype=np.int32)
    for k in range(4):
        cells[:, k] = np.floor((bv[:, k] - offset[k % 2]) / stride[k % 2])
    cells[:, :2] = np.maximum(cells[:, :2], 0)
    cells[:, 2] = np.minimum(cells[:, 2], nx - 1)
    cells[:, 3] = np.minimum(cells[:, 3], ny - 1)
    if (cells[:, 0] > nx - 1).any() or (cells[:, 1] > ny - 1).any() or (cells[:, 2:] < 0).any():
        raise _lib.PapcError("anchor_cache: an anchor lies wholly outside the pillar grid (%d x %d cells); the source would index the map "
                             "from its far end there" % (nx, ny))
    return cells


class TargetAssigner:
    """core/target_assigner.py with the box coder's two switches (``encode_angle_to_vector``, ``smooth_dim``) and NearestIouSimilarity built in"""

    def __init__(self, anchor_generators, positive_fraction=None, sample_size=512, encode_angle_to_vector=False, smooth_dim=False):
        self._anchor_generators = list(anchor_generators)
        self._positive_fraction, self._sample_size = positive_fraction, sample_size
        self.encode_angle_to_vector, self.smooth_dim = bool(encode_angle_to_vector), bool(smooth_dim)

    @property
    def code_size(self):
        return 8 if self.encode_angle_to_vector else 7

    @property
    def num_anchors_per_location(self):
        return sum(g.num_anchors_per_localization for g in self._anchor_generators)

    def generate_anchors(self, feature_map_size):
        """(D, H, W) -> {"anchors" [D,H,W,n,7], "matched_thresholds", "unmatched_thresholds" [A]} (target_assigner.py:58-85).  The anchors of the
        generators are concatenated on axis -2, the threshold vectors on axis 0, as the source writes it."""
        anchors_list, match_list, unmatch_list = [], [], []
        for gen in self._anchor_generators:
            anchors = gen.generate(feature_map_size)
            anchors = anchors.reshape(anchors.shape[:3] + (-1, 7))
            anchors_list.append(anchors)
            n = int(np.prod(anchors.shape[:-1]))
            match_list.append(np.full([n], gen.match_threshold, anchors.dtype))
            unmatch_list.append(np.full([n], gen.unmatch_threshold, anchors.dtype))
        return {"anchors": np.concatenate(anchors_list, axis=-2), "matched_thresholds": np.concatenate(match_list, axis=0),
                "unmatched_thresholds": np.concatenate(unmatch_list, axis=0)}

    def anchor_cache(self, feature_map_size, voxel_size, point_cloud_range, grid_size, device=None):
        return anchor_cache(self, feature_map_size, voxel_size, point_cloud_range, grid_size, device)

    def assign(self, cache, gt_boxes, gt_classes, num_gt, anchors_mask=None, **kw):
        return assign(cache, gt_boxes, gt_classes, num_gt, anchors_mask, **kw)


def anchor_cache(assigner, feature_map_size, voxel_size, point_cloud_range, grid_size, device=None):
    """Everything static about the anchors, computed once on the host (preprocess.py:253-265) and held as device tensors: ``anchors`` [A,7],
    ``anchors_bv`` [A,4] (their near-bboxes), ``cells`` [A,4] int32 (anchor_cells), ``matched_thresholds`` / ``unmatched_thresholds`` [A], with
    ``grid_size`` (nx, ny) and the assigner's switches.  feature_map_size (D, H, W); voxel_size, point_cloud_range, grid_size as the voxel
    generator has them (x, y, z order)."""
    ret = assigner.generate_anchors(feature_map_size)
    anchors = np.ascontiguousarray(ret["anchors"].reshape(-1, 7), dtype=np.float32)
    bv = rbbox2d_to_near_bbox(torch.from_numpy(anchors[:, [0, 1, 3, 4, 6]])).contiguous()
    cells = anchor_cells(bv.numpy(), voxel_size, point_cloud_range, grid_size)
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu") if device is None else torch.device(device)
    f32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)       # noqa: E731
    return {"anchors": f32(anchors), "anchors_bv": bv.to(dev), "cells": torch.from_numpy(cells).to(dev),
            "matched_thresholds": f32(ret["matched_thresholds"]), "unmatched_thresholds": f32(ret["unmatched_thresholds"]),
            "grid_size": (int(grid_size[0]), int(grid_size[1])), "feature_map_size": tuple(int(v) for v in feature_map_size),
            "encode_angle_to_vector": assigner.encode_angle_to_vector, "smooth_dim": assigner.smooth_dim,
            "positive_fraction": assigner._positive_fraction}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the anchor mask

def mask_workspace_bytes(B, A, ny, nx):
    """bytes of workspace one anchors_mask call of this shape needs (papc_anchors_mask_workspace); raises PapcError outside the kernels' limits"""
    return _lib.workspace_bytes("papc_anchors_mask_workspace", AnchorsMaskDesc(B=B, A=A, ny=ny, nx=nx))


def _mask_torch(coors, B, cells, nx, ny, thresh):
    """preprocess.py:271-278 for B frames at once: counts (float32, as the source's map), cumsum over y then x, the four-corner expression"""
    c = coors.long()
    ok = (c[:, 0] >= 0) & (c[:, 0] < B) & (c[:, 2] >= 0) & (c[:, 2] < ny) & (c[:, 3] >= 0) & (c[:, 3] < nx)
    c = c[ok]
    dense = torch.zeros(B * ny * nx, dtype=torch.float32, device=coors.device)
    dense.index_add_(0, (c[:, 0] * ny + c[:, 2]) * nx + c[:, 3], torch.ones(c.shape[0], dtype=torch.float32, device=coors.device))
    S = dense.view(B, ny, nx).cumsum(1).cumsum(2)
    x1, y1, x2, y2 = (cells[:, k].long() for k in range(4))
    area = S[:, y2, x2] - S[:, y2, x1] - S[:, y1, x2] + S[:, y1, x1]                  # ID - IB - IC + IA (box_np_ops.py:800-804)
    return (area > thresh).to(torch.uint8)


def anchors_mask(coors, batch_size, cache, anchor_area_threshold=1, out=None, workspace=None, fused=None):
    """coors [P,4] int = (batch, z, y, x) (what PointPillarsScatter.forward takes; rows with a batch index outside [0, batch_size) are ignored,
    so -1 pads), cache from anchor_cache -> mask [B,A] uint8: 1 where the anchor's cell box holds more than ``anchor_area_threshold`` pillars by
    the source's four-corner expression.  ``out`` ([B,A] uint8) and ``workspace`` (uint8, >= mask_workspace_bytes(...)) may be passed in for
    reuse.  ``fused``: None = as PAPC_DET_TARGETS says, False = the torch-op flavour, True = the kernels."""
    B, cells = int(batch_size), cache["cells"]
    A, (nx, ny) = int(cells.shape[0]), cache["grid_size"]
    assert coors.dim() == 2 and coors.shape[1] == 4, "coors [P,4] = (batch, z, y, x) expected"
    dev = cells.device
    if out is None:
        out = torch.empty((B, A), dtype=torch.uint8, device=dev)
    assert out.shape == (B, A) and out.dtype == torch.uint8 and out.is_contiguous(), "out: [B,A] uint8 expected"
    if not _use_fused(fused):
        out.copy_(_mask_torch(coors.to(dev), B, cells, nx, ny, float(anchor_area_threshold)))
        return out
    if not (coors.is_cuda and cells.is_cuda and out.is_cuda):
        raise _lib.PapcError("anchors_mask needs CUDA (ROCm) tensors: there is no CPU fallback (PAPC_DET_TARGETS=0 selects the torch-op flavour)")
    coors = coors.int().contiguous()
    lib = _lib.load()
    d = AnchorsMaskDesc(B=B, A=A, ny=ny, nx=nx, P=int(coors.shape[0]), area_thresh=float(anchor_area_threshold))
    ws, _ = _lib.workspace("papc_anchors_mask_workspace", d, dev, workspace)
    io = AnchorsMaskIo(coors=ptr(coors) if coors.shape[0] else None, cells=ptr(cells), mask=ptr(out))
    check(lib.papc_anchors_mask_u8(ctypes.byref(d), ctypes.byref(io), ptr(ws), ws.numel(), stream_ptr()), "papc_anchors_mask_u8")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# second_box_encode and assign

def second_box_encode(boxes, anchors, encode_angle_to_vector=False, smooth_dim=False, fused=None):
    """box_np_ops.py:30: boxes [..., 7] (x, y, z, w, l, h, r), anchors [..., 7] -> encodings [..., 7] ([..., 8] with encode_angle_to_vector);
    boxcodec.second_box_encode under this module's switch."""
    return boxcodec.second_box_encode(boxes, anchors, encode_angle_to_vector, smooth_dim, _use_fused(fused))


def assign_workspace_bytes(B, A, Gmax, encode_angle_to_vector=False):
    """bytes of workspace one assign call of this shape needs (papc_det_assign_workspace); raises PapcError outside the kernels' limits"""
    d = DetAssignDesc(B=B, A=A, Gmax=Gmax, encode_angle_to_vector=int(bool(encode_angle_to_vector)), code_size=8 if encode_angle_to_vector else 7)
    return _lib.workspace_bytes("papc_det_assign_workspace", d)


def _iou_torch(bv, qbv):
    """iou_jit (box_np_ops.py:654-682) with eps = 0, vectorised: bv [N,4], qbv [K,4] -> [N,K], each element by the source's operations in order"""
    a, q = bv[:, None, :], qbv[None, :, :]
    qarea = (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
    iw = torch.minimum(a[..., 2], q[..., 2]) - torch.maximum(a[..., 0], q[..., 0])
    ih = torch.minimum(a[..., 3], q[..., 3]) - torch.maximum(a[..., 1], q[..., 1])
    ua = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + qarea - iw * ih
    return torch.where((iw > 0) & (ih > 0), iw * ih / ua, torch.zeros_like(ua))


def _assign_frame_torch(cache, gt, cls, inside, res, b):
    """create_target_np (target_ops.py:86-191, positive_fraction=None) for one frame on the anchors ``inside`` (indices); writes row b of ``res``"""
    anchors, bv = cache["anchors"][inside], cache["anchors_bv"][inside]
    n, G = int(inside.shape[0]), int(gt.shape[0])
    if n == 0:
        return
    if G == 0:
        res["labels"][b, inside] = 0                                                  # :155-156
        return
    ov = _iou_torch(bv, rbbox2d_to_near_bbox(gt[:, [0, 1, 3, 4, 6]]))
    amax = ov.max(dim=1).values
    cols = torch.arange(G, device=ov.device).expand_as(ov)
    aarg = torch.where(ov == amax[:, None], cols, G).min(dim=1).values                # np.argmax: the first of equal maxima
    gmax = ov.max(dim=0).values
    gmax = torch.where(gmax == 0, -torch.ones_like(gmax), gmax)                       # :109-110
    force = (ov == gmax[None, :]).any(dim=1)                                          # :113-114
    own = cls[aarg].to(torch.int32)
    lab = torch.full((n,), -1, dtype=torch.int32, device=ov.device)
    lab = torch.where(amax >= cache["matched_thresholds"][inside], own, lab)          # :121-123
    lab = torch.where(amax < cache["unmatched_thresholds"][inside], torch.zeros_like(lab), lab)       # :125, :158
    lab = torch.where(force, own, lab)                                                # :117-118, :160
    fg = lab > 0
    res["labels"][b, inside] = lab
    res["max_overlap"][b, inside] = amax
    res["gt_ids"][b, inside] = torch.where(fg, aarg.to(torch.int32), torch.full_like(lab, -1))
    res["reg_weights"][b, inside] = fg.to(torch.float32)
    if bool(fg.any()):
        res["reg_targets"][b, inside[fg]] = _encode_torch(gt[aarg[fg]], anchors[fg], cache["encode_angle_to_vector"], cache["smooth_dim"])
    res["num_pos"][b] = int(fg.sum())


def assign(cache, gt_boxes, gt_classes, num_gt, anchors_mask=None, out=None, workspace=None, fused=None):
    """TargetAssigner.assign for a padded batch.  cache from anchor_cache; gt_boxes [B,Gmax,7], gt_classes [B,Gmax] int (classes count from 1),
    num_gt [B] int -- rows >= num_gt[b] are never read into a decision; anchors_mask [B,A] (anchors_mask()'s bytes) or None.  Returns a dict:
    labels [B,A] int32 (-1 don't care, 0 negative, k > 0 class k), reg_targets [B,A,7|8], reg_weights [B,A], gt_ids [B,A] int32 (the assigned
    gt where label > 0, else -1), max_overlap [B,A] (the anchor's best overlap; 0 outside the mask), num_pos [B] int32.  ``out`` (a dict of the
    output tensors) and ``workspace`` (uint8, >= assign_workspace_bytes(...)) may be passed in for reuse.  No host synchronisation on the
    fused path."""
    if cache.get("positive_fraction") is not None:
        raise _lib.PapcError("assign: positive_fraction is not built -- the source samples with numpy's global RNG, no parity can be stated")
    anchors = cache["anchors"]
    A, dev = int(anchors.shape[0]), anchors.device
    B, Gmax = int(gt_boxes.shape[0]), int(gt_boxes.shape[1])
    assert gt_boxes.shape == (B, Gmax, 7) and gt_classes.shape == (B, Gmax) and num_gt.shape == (B,), "gt_boxes [B,Gmax,7], gt_classes [B,Gmax], num_gt [B]"
    angle_vec, smooth = cache["encode_angle_to_vector"], cache["smooth_dim"]
    code = 8 if angle_vec else 7
    mask = None if anchors_mask is None else anchors_mask.reshape(B, A)
    use_fused = _use_fused(fused)
    if use_fused and not (anchors.is_cuda and gt_boxes.is_cuda and gt_classes.is_cuda and num_gt.is_cuda and (mask is None or mask.is_cuda)):
        raise _lib.PapcError("assign needs CUDA (ROCm) tensors: there is no CPU fallback (PAPC_DET_TARGETS=0 selects the torch-op flavour)")
    if Gmax > GMAX_LIMIT:
        raise _lib.PapcError("assign: Gmax=%d not in [0, %d]" % (Gmax, GMAX_LIMIT))
    res = _lib.outputs({} if out is None else out,
                       (("labels", torch.int32, (B, A)), ("reg_targets", torch.float32, (B, A, code)), ("reg_weights", torch.float32, (B, A)),
                        ("gt_ids", torch.int32, (B, A)), ("max_overlap", torch.float32, (B, A)), ("num_pos", torch.int32, (B,))), dev)

    if not use_fused:
        res["labels"].fill_(-1), res["gt_ids"].fill_(-1)
        res["reg_targets"].zero_(), res["reg_weights"].zero_(), res["max_overlap"].zero_(), res["num_pos"].zero_()
        counts = num_gt.tolist()
        gt_boxes, gt_classes = gt_boxes.float().to(dev), gt_classes.to(dev)
        for b in range(B):
            G = min(max(int(counts[b]), 0), Gmax)
            inside = torch.arange(A, device=dev) if mask is None else torch.nonzero(mask[b].to(dev) != 0).reshape(-1)
            _assign_frame_torch(cache, gt_boxes[b, :G], gt_classes[b, :G], inside, res, b)
        return res

    gt_boxes, gt_classes, num_gt = gt_boxes.contiguous().float(), gt_classes.int().contiguous(), num_gt.int().contiguous()
    if mask is not None:
        mask = mask.contiguous() if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8).contiguous()
    lib = _lib.load()
    d = DetAssignDesc(B=B, A=A, Gmax=Gmax, encode_angle_to_vector=int(angle_vec), smooth_dim=int(smooth), code_size=code)
    ws, _ = _lib.workspace("papc_det_assign_workspace", d, dev, workspace)
    io = DetAssignIo(anchors=ptr(anchors), anchors_bv=ptr(cache["anchors_bv"]), matched=ptr(cache["matched_thresholds"]),
                     unmatched=ptr(cache["unmatched_thresholds"]), anchors_mask=ptr(mask), gt_boxes=ptr(gt_boxes) if Gmax else None,
                     gt_classes=ptr(gt_classes) if Gmax else None, num_gt=ptr(num_gt), labels=ptr(res["labels"]),
                     reg_targets=ptr(res["reg_targets"]), reg_weights=ptr(res["reg_weights"]), gt_ids=ptr(res["gt_ids"]),
                     max_overlap=ptr(res["max_overlap"]), num_pos=ptr(res["num_pos"]))
    check(lib.papc_det_assign_f32(ctypes.byref(d), ctypes.byref(io), ptr(ws), ws.numel(), stream_ptr()), "papc_det_assign_f32")
    return res
