"""Regenerates tests/golden/ref_dettarget.npz: what the REFERENCE'S OWN target pipeline computes on the scenes of tests/dettarget_cases.py --
create_anchors_3d_stride / create_anchors_3d_range behind its anchor generators, TargetAssigner.generate_anchors, rbbox2d_to_near_bbox,
sparse_sum_for_anchors_mask + the two cumsums + fused_get_anchors_area, and TargetAssigner.assign -> create_target_np with NearestIouSimilarity
and second_box_encode.  Needs a checkout of the reference; only arrays are committed, next to the inputs they were computed from.

    python tests/golden/make_dettarget_golden.py /path/to/reference          (the directory that holds PAPC/)

The reference's modules import numba and three compiled helpers that this pipeline never calls; they are replaced by in-memory stand-ins here
(numba.jit = identity, empty modules; the ``core`` package is entered without its __init__, which imports paddle), and np.meshgrid is wrapped to return the list the source assigns into.  Every scene's purpose is asserted
on the reference's outputs, so a scene cannot lose it silently.  Running it twice gives byte-identical files.
"""
import io
import os
import sys
import types
import zipfile

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import dettarget_cases as C                                   # noqa: E402


def _stand_ins(root):
    core = types.ModuleType("core")                                      # the package without its __init__ (which imports paddle and the data
    core.__path__ = [os.path.join(root, "core")]                         # loaders): its modules are still the reference's own files
    sys.modules["core"] = core

    def jit(*args, **kw):
        if len(args) == 1 and callable(args[0]) and not kw:
            return args[0]
        return lambda f: f
    numba = types.ModuleType("numba")
    numba.jit = numba.njit = jit
    sys.modules["numba"] = numba
    for name, attrs in (("libs.tools.buildtools.pybind11_build", ("load_pb11",)), ("libs.ops.non_max_suppression.nms_gpu", ("rotate_iou_gpu_eval",)),
                        ("libs.ops.geometry", ("points_in_convex_polygon_3d_jit",)), ("libs.ops.box_ops_cc", ())):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, None)
        sys.modules[name] = m
    meshgrid = np.meshgrid
    np.meshgrid = lambda *a, **kw: list(meshgrid(*a, **kw))


class _Logged(np.ndarray):
    """the dense map with every element read written down: fused_get_anchors_area keeps its cell box to itself"""
    log = []

    def __getitem__(self, idx):
        if isinstance(idx, tuple) and len(idx) == 2:
            _Logged.log.append((int(idx[0]), int(idx[1])))
        return np.asarray(self).__getitem__(idx)


def record(ref, name, s):
    from core.anchor_generator import AnchorGeneratorRange, AnchorGeneratorStride
    from core.similarity_calculator import NearestIouSimilarity
    from core.target_assigner import TargetAssigner
    from libs.ops import box_np_ops

    angle_vec, smooth = s["angle_vec"], s["smooth"]
    code = 8 if angle_vec else 7

    class Coder:
        code_size = code

        @staticmethod
        def encode(boxes, anchors):
            return box_np_ops.second_box_encode(boxes, anchors, angle_vec, smooth)

    class Similarity(NearestIouSimilarity):
        last = None

        def _compare(self, boxes1, boxes2):
            Similarity.last = NearestIouSimilarity._compare(self, boxes1, boxes2)
            return Similarity.last

    gens = [(AnchorGeneratorStride if kind == "stride" else AnchorGeneratorRange)(**kw) for kind, kw in s["gens"]]
    assigner = TargetAssigner(Coder, gens, region_similarity_calculator=Similarity())
    ret = assigner.generate_anchors(list(s["fmap"]))
    anchors = ret["anchors"].reshape([-1, 7])
    assert anchors.dtype == np.float32
    matched, unmatched = ret["matched_thresholds"], ret["unmatched_thresholds"]
    bv = box_np_ops.rbbox2d_to_near_bbox(anchors[:, [0, 1, 3, 4, 6]])
    assert bv.dtype == np.float32
    A, B = anchors.shape[0], len(s["num_gt"])
    grid = np.array(s["grid_size"])
    out = {k: s[k] for k in C.INPUT_KEYS}
    out.update(anchors=ret["anchors"], matched_thresholds=matched, unmatched_thresholds=unmatched, anchors_bv=bv,
               area=np.zeros((B, A), np.float32), mask=np.zeros((B, A), np.uint8), labels=np.zeros((B, A), np.int32),
               reg_targets=np.zeros((B, A, code), np.float32), reg_weights=np.zeros((B, A), np.float32), gt_ids=np.full((B, A), -1, np.int32),
               max_overlap=np.zeros((B, A), np.float32), num_pos=np.zeros(B, np.int32))
    force_counts = []
    for b in range(B):
        coors = s["coors"][s["coors"][:, 0] == b][:, 1:]                 # the frame's own (z, y, x) rows, as the voxel generator hands them over
        dense = box_np_ops.sparse_sum_for_anchors_mask(coors, tuple(grid[::-1][1:]))
        dense = dense.cumsum(0)
        dense = dense.cumsum(1)
        _Logged.log = []
        area = box_np_ops.fused_get_anchors_area(dense.view(_Logged), bv, s["voxel_size"], s["pc_range"], grid)
        reads = np.array(_Logged.log, np.int32).reshape(A, 4, 2)         # ID (y2, x2), IA (y1, x1), IB (y2, x1), IC (y1, x2)
        cells = np.stack([reads[:, 1, 1], reads[:, 1, 0], reads[:, 0, 1], reads[:, 0, 0]], axis=1)
        assert (reads[:, 2] == np.stack([cells[:, 3], cells[:, 0]], 1)).all() and (reads[:, 3] == np.stack([cells[:, 1], cells[:, 2]], 1)).all()
        assert "cells" not in out or (out["cells"] == cells).all()
        out["cells"] = cells
        mask = area > s["area_thr"]
        out["area"][b], out["mask"][b] = area, mask
        G = int(s["num_gt"][b])
        gt, cls = s["gt_boxes"][b, :G], s["gt_classes"][b, :G]
        Similarity.last = None
        t = assigner.assign(anchors, gt, mask, gt_classes=cls, matched_thresholds=matched, unmatched_thresholds=unmatched)
        out["labels"][b], out["reg_targets"][b], out["reg_weights"][b] = t["labels"], t["bbox_targets"], t["bbox_outside_weights"]
        out["gt_ids"][b, t["assigned_anchors_inds"]] = t["positive_gt_id"]
        out["num_pos"][b] = len(t["assigned_anchors_inds"])
        inside = np.where(mask)[0]
        if Similarity.last is not None:
            ov = Similarity.last
            assert ov.dtype == np.float32 and ov.shape == (len(inside), G)
            out["max_overlap"][b, inside] = ov.max(axis=1)
            gmax = ov.max(axis=0)
            force_counts.append([(int((ov[:, g] == gmax[g]).sum()) if gmax[g] > 0 else 0) for g in range(G)])
            s.setdefault("_ov", {})[b] = (inside, ov)
        assert (out["labels"][b][~mask] == -1).all() and (out["reg_weights"][b] == (out["labels"][b] > 0)).all()
    check_purpose(name, s, out, force_counts)
    return out


def check_purpose(name, s, o, force_counts):
    A = o["mask"].shape[1]
    lab = o["labels"]
    if name in ("a", "f01", "f10", "f11"):
        assert A == 798 and 0.6 < o["mask"].mean() < 0.8, o["mask"].mean()
        assert all((lab == v).any() for v in (-1, 0, 1)) and ((lab == -1) & (o["mask"] != 0)).any()
        assert o["reg_targets"].shape[-1] == (8 if s["angle_vec"] else 7)
    if name == "b":
        inside, ov = s["_ov"][0]
        fc = force_counts[0]
        assert fc[0] >= 2 and o["max_overlap"].max() == 1.0 and fc[2] == 0 and ov[:, 2].max() == 0, fc
        gmax = ov.max(axis=0)
        aarg = ov.argmax(axis=1)
        forced_by_3 = ov[:, 3] == gmax[3]
        assert (forced_by_3 & (aarg != 3) & (s["gt_classes"][0][aarg] == 1)).any()      # forced by a class-2 gt, labelled by its own class-1 argmax
        assert (lab[0][inside][forced_by_3 & (aarg == 0)] == 1).all() and (forced_by_3 & (aarg == 0)).any()
        assert gmax[4] < 1.0 and o["mask"][0, (12 * 24 + 20) * 2] == 0 and (o["anchors"].reshape(-1, 7)[(12 * 24 + 20) * 2] == s["gt_boxes"][0, 4]).sum() >= 6
        assert (lab == 2).any() and (lab == 1).any()
    if name == "c":
        assert tuple(s["num_gt"]) == (33, 0, 1) and o["mask"][2].sum() == 0 and o["mask"][0].any() and o["mask"][1].any()
        assert (lab[1][o["mask"][1] != 0] == 0).all() and (lab[2] == -1).all() and o["num_pos"][0] > 0 and np.isnan(s["gt_boxes"][1]).all()
    if name == "d":
        assert A == 4400
        inside, ov = s["_ov"][0]
        blocks = [set((inside[ov[:, g] > 0] // 256).tolist()) for g in range(ov.shape[1])]
        assert max(len(bl) for bl in blocks) >= 3, blocks              # the per-gt maximum is taken across workgroups of 256 anchors
    if name == "e":
        n1 = 2
        per_anchor = np.tile(np.array([0.6] * n1 + [0.5] * 2, np.float32), A // 4)
        assert (o["matched_thresholds"] != per_anchor).any() and o["anchors"].shape[-2] == 4       # the vectors do not follow the anchors' order
        assert (lab > 0).any()
    if name in ("g0", "g1"):
        c = o["cells"]
        assert (c[:, 0] == 0).any() and (c[:, 2] == 37).any() and (c[:, 1] == 0).any() and (c[:, 3] == 41).any()
        assert (s["coors"][:, 0] == -1).sum() == 7 and o["area"].max() >= 2 and 0 < o["mask"].mean() < 1
        assert ((o["area"] > 0) & (o["area"] <= 1)).any()               # thresholds 0 and 1 give different masks


def main():
    ref = os.path.abspath(sys.argv[1])
    root = os.path.join(ref, "PAPC", "models", "detect", "pointpillars")
    sys.path.insert(0, root)
    _stand_ins(root)
    blob = {}
    for name, make in C.SCENES.items():
        out = record(ref, name, make())
        for k in C.INPUT_KEYS + C.OUTPUT_KEYS:
            blob["%s.%s" % (name, k)] = out[k]
        print("%-4s A=%-5d inside %.2f  labels -1/0/+ %s  num_pos %s" % (name, out["mask"].shape[1], out["mask"].mean(),
              [int((out["labels"] == -1).sum()), int((out["labels"] == 0).sum()), int((out["labels"] > 0).sum())], out["num_pos"].tolist()))
    assert (blob["g0.mask"] != blob["g1.mask"]).any()
    path = os.path.join(HERE, "ref_dettarget.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:          # fixed dates and order: the same bytes on every run
        for k in sorted(blob):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(blob[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    print("wrote %s (%d bytes)" % (os.path.basename(path), size))


if __name__ == "__main__":
    main()
