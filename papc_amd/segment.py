"""The first seg_net layer of the PointNet part segmenters on the library's kernels: relu(bn(conv(concat([point_feat, tile(global_feat, N)])))).

Reference: PAPC/models/segment/pointnet/pointnet.py:103-107 and segment/pointnet_base/pointnet_base.py:31-35
    x = concat([point_feat [B, 64, N], tile(global_feat [B, Cg, 1], N)]);   seg_net[0..2] = Conv1D(64 + Cg, 512, 1), BatchNorm(512), ReLU
The layer itself -- the autograd node, the BatchNorm sequence, the checks -- is cloudconcat.concat_bn_relu; this module names its kernel family,
the Cp = 64 one of csrc/cloud_concat.hip (the segmenters stay on it even where the K-looped family of vfe.py would take the shape too).

PAPC_SEG_CONCAT=0 (read once, at import) materialises the concat with copyops.cat_copy and runs it as the first layer of a shared-MLP stack
(mlp.shared_mlp_max, x_rows 64 + Cg wide): a second, independent implementation that the tests compare against and the benchmark's baseline.
Widths outside the kernel's shapes (Cg not a multiple of 64 in 64..1024) take that path as well.  CPU tensors raise PapcError.
"""
import os

from .cloudconcat import Family, concat_bn_relu

_SEG_CONCAT = os.environ.get("PAPC_SEG_CONCAT", "1") != "0"   # A/B switch: 0 = the materialised concat on the shared-MLP stack


def kernel_ok(cp, cg, cout):
    """whether csrc/cloud_concat.hip takes this layer (papc_cloud_concat_conv_f32's shapes)"""
    return cp == 64 and cout == 512 and 64 <= cg <= 1024 and cg % 64 == 0


FAMILY = Family("papc_cloud_concat_conv_parts", "papc_cloud_concat_conv_f32", "papc_cloud_concat_conv_bwd_workspace",
                "papc_cloud_concat_conv_bwd_f32", kernel_ok)


def cloud_concat_bn_relu(point_rows, global_feat, conv, bn, N, training):
    """seg_net[0..2] of the PointNet segmenters: point_rows [B*N, 64] (point-major), global_feat [B, Cg], conv = nn.Conv1d(64 + Cg, 512, 1)
    (its [512, 64 + Cg, 1] weight read in place), bn = its nn.BatchNorm1d(512) -> relu(bn(conv(concat([point, tile(global, N)])))) [B*N, 512].
    Gradients reach point_rows, global_feat, conv.weight / bias and bn.weight / bias; training=True updates bn's running statistics."""
    return concat_bn_relu("cloud_concat_bn_relu", FAMILY, _SEG_CONCAT, point_rows, global_feat, conv, bn, N, training)
