"""The wide concat layers of the VFE models on the library's kernels: relu(bn(conv(concat([point_rows, tile(global_feat, N)])))).

Reference: PAPC/models/classify/vfe/vfe.py:79-83 (vfe.pointnet_2.mlp_1.0 = Conv1D(512, 64, 1) + BatchNorm + ReLU over concat([x1, tile(max x1)]))
and PAPC/models/segment/vfe/vfe.py:33-36 (seg_net[0..2] = Conv1D(max_points + 512, 512, 1) + BatchNorm + ReLU over concat([x1, tile(max x1), tile(x2)])).
The layer itself -- the autograd node, the BatchNorm sequence, the checks -- is cloudconcat.concat_bn_relu, as segment.cloud_concat_bn_relu; this
module names its kernel family, the K-looped one of csrc/cloud_concat_k.hip.

PAPC_VFE_CONCAT=0 (read once, at import) materialises the concat with copyops.cat_copy and runs it as a one-layer shared-MLP stack
(mlp.shared_mlp_max, pool=False): a second, independent implementation that the tests compare against and the benchmark's baseline.  Widths
papc_cloud_concat_k_ok refuses take that path as well.  CPU tensors and non-float32 tensors raise PapcError.
"""
import os

from . import _lib
from .cloudconcat import Family, concat_bn_relu

_VFE_CONCAT = os.environ.get("PAPC_VFE_CONCAT", "1") != "0"   # A/B switch: 0 = the materialised concat on the shared-MLP stack


def kernel_ok(cp, cg, cout):
    """whether csrc/cloud_concat_k.hip takes this layer (papc_cloud_concat_k_ok)"""
    return bool(_lib.load().papc_cloud_concat_k_ok(int(cp), int(cg), int(cout)))


FAMILY = Family("papc_cloud_concat_k_parts", "papc_cloud_concat_k_f32", "papc_cloud_concat_k_bwd_workspace", "papc_cloud_concat_k_bwd_f32",
                kernel_ok)


def concat_k_bn_relu(point_rows, global_feat, conv, bn, N, training):
    """point_rows [B*N, Cp] (point-major), global_feat [B, Cg], conv = nn.Conv1d(Cp + Cg, Cout, 1) (its [Cout, Cp + Cg, 1] weight read in place),
    bn = its nn.BatchNorm1d(Cout) -> relu(bn(conv(concat([point, tile(global, N)])))) [B*N, Cout].  Gradients reach point_rows, global_feat,
    conv.weight / bias and bn.weight / bias; training=True updates bn's running statistics."""
    return concat_bn_relu("concat_k_bn_relu", FAMILY, _VFE_CONCAT, point_rows, global_feat, conv, bn, N, training)
