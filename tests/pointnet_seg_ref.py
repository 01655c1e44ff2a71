"""Float64 restatement of the PointNet part segmenters (/root/reference/PAPC/models/segment/pointnet/pointnet.py:4-114 and
segment/pointnet_base/pointnet_base.py:4-80), for the GPU tests of papc_amd.models.PointNet_Seg / PointNet_Basic_Seg.  Plain torch on CPU
tensors, the concat materialised as the source forms it; autograd gives the reference gradients.

Parameters come as a dict of this package's state names -> float64 tensors (running statistics too, for eval mode).  ``dec`` optionally pins
the discontinuous decisions to the kernels' own, per stack as in tests/pointnet_ref.py; ``dec["seg0"]`` = (None, alive, None) pins the ReLU
of seg_net[0..2] (alive [B*N, 512] bool), ``dec["seg1"]`` the stack seg_net[3..11]."""
import torch

from tests import pointnet_ref


def seg_head(P, point_rows, g, N, train, dec, eps=1e-5, tally=None):
    """concat([point, tile(global, N)]) -> seg_net (pointnet.py:110-114) -> logits [B, N, num_classes]"""
    B = g.shape[0]
    rows = torch.cat([point_rows, g.repeat_interleave(N, 0)], 1)                                   # :110-111 (point-major rows)
    h = pointnet_ref.stack(P, "seg_net", [0], rows, N, False, eps, train, dec.get("seg0"), tally)        # seg_net[0..2]
    h = pointnet_ref.stack(P, "seg_net", [3, 6, 9], h, N, False, eps, train, dec.get("seg1"), tally)     # seg_net[3..11]
    w, b = P["seg_net.12.weight"].squeeze(-1), P["seg_net.12.bias"]
    return (h @ w.t() + b).reshape(B, N, -1)                                                       # seg_net[12], :112-113


def pointnet_seg(P, x, train=True, dec=None, eps=1e-5, tally=None):
    """x [B, 3, N] float64 -> logits [B, N, num_classes]; pointnet.py:84-114 step by step"""
    dec = dec or {}
    B, _, N = x.shape
    pts0 = x.transpose(1, 2)
    g = pointnet_ref.stack(P, "input_transform_net", [0, 3, 6], pts0.reshape(B * N, 3), N, True, eps, train, dec.get("input_transform_net"), tally)
    t = pointnet_ref.fc_block(P, "input_fc", g, [0, 2, 4], dec.get("input_fc"), tally=tally).reshape(B, 3, 3)
    pts = torch.bmm(pts0, t)
    h = pointnet_ref.stack(P, "mlp_1", [0, 3], pts.reshape(B * N, 3), N, False, eps, train, dec.get("mlp_1"), tally)
    g = pointnet_ref.stack(P, "feature_transform_net", [0, 3, 6], h, N, True, eps, train, dec.get("feature_transform_net"), tally)
    t = pointnet_ref.fc_block(P, "feature_fc", g, [0, 2, 4], dec.get("feature_fc"), tally=tally).reshape(B, 64, 64)
    point_feat = torch.bmm(h.reshape(B, N, 64), t).reshape(B * N, 64)
    g = pointnet_ref.stack(P, "mlp_2", [0, 3, 6], point_feat, N, True, eps, train, dec.get("mlp_2"), tally)
    return seg_head(P, point_feat, g, N, train, dec, eps, tally)


def pointnet_basic_seg(P, x, train=True, dec=None, eps=1e-5, tally=None):
    """x [B, 3, N] float64 -> logits [B, N, num_classes]; pointnet_base.py:24-39, :66-76"""
    dec = dec or {}
    B, _, N = x.shape
    h = pointnet_ref.stack(P, "pointnet_bacic.mlp_1", [0, 3], x.transpose(1, 2).reshape(B * N, 3), N, False, eps, train, dec.get("mlp_1"), tally)
    g = pointnet_ref.stack(P, "pointnet_bacic.mlp_2", [0, 3, 6], h, N, True, eps, train, dec.get("mlp_2"), tally)
    return seg_head(P, h, g, N, train, dec, eps, tally)
