"""Float64 restatement of the VFE models (PAPC/models/classify/vfe/vfe.py:5-86 and PAPC/models/segment/vfe/vfe.py:5-97), for the GPU tests of
papc_amd.models.VFE_Clas / VFE_Seg.  Plain torch on CPU tensors, both concats materialised as the source forms them; autograd gives the
reference gradients.

Parameters come as a dict of this package's state names -> float64 tensors (running statistics too, for eval mode).  ``dec`` optionally pins
the discontinuous decisions to the kernels' own, per stack ``(argmax, alive, masks)`` as in tests/pointnet_ref.py:
  ``pointnet_1``  the five layers of vfe.pointnet_1 (every row kept)        ``g1``       argmax [B, C] of the max over each cloud's x1 rows
  ``concat0``     vfe.pointnet_2.mlp_1.0 on the concat: (None, alive, None)  ``pointnet_2``  the other four layers of vfe.pointnet_2, pooled
  ``seg0``        seg_net[0..2] on the wide concat: (None, alive, None)      ``seg1``     the stack seg_net[3..11]
  ``fc``          the classifier's FC block: (mask1, mask2, keep)"""
import torch

from tests import pointnet_ref, torch_ref

P1 = ["vfe.pointnet_1.mlp_1.0", "vfe.pointnet_1.mlp_1.1", "vfe.pointnet_1.mlp_2.0", "vfe.pointnet_1.mlp_2.1", "vfe.pointnet_1.mlp_2.2"]
P2 = ["vfe.pointnet_2.mlp_1.0", "vfe.pointnet_2.mlp_1.1", "vfe.pointnet_2.mlp_2.0", "vfe.pointnet_2.mlp_2.1", "vfe.pointnet_2.mlp_2.2"]


def blocks(P, names, rows, N, pool, eps, train, dec=None):
    """relu(bn(conv)) over the ConvBNReLU blocks ``names``; rows [B*N, Cin]; pool: the max over each cloud's N rows"""
    params = [(P[n + "._conv.weight"].squeeze(-1), P[n + "._conv.bias"], P[n + "._batch_norm.weight"], P[n + "._batch_norm.bias"]) for n in names]
    running = None if train else [(P[n + "._batch_norm.running_mean"], P[n + "._batch_norm.running_var"]) for n in names]
    argmax, alive, masks = dec if dec is not None else (None, None, None)
    if pool:
        return torch_ref.stack_routed(rows, params, N, eps, argmax, alive, masks, running=running)[0]
    am = torch.zeros(rows.shape[0], params[-1][0].shape[0], dtype=torch.long) if alive is not None else None
    return torch_ref.stack_routed(rows, params, 1, eps, am, alive, masks, running=running)[0]


def features(P, x, train, dec, eps=1e-5):
    """VFE.forward (classify :72-86, segment :83-97) -> (the [B*N, 2C] concat the source calls x1, x2 = the pooled pointnet_2 [B, max_points])"""
    B, _, N = x.shape
    x1 = blocks(P, P1, x.transpose(1, 2).reshape(B * N, 3), N, False, eps, train, dec.get("pointnet_1"))
    C = x1.shape[1]
    am = dec.get("g1")
    xg = x1.reshape(B, N, C)
    g1 = xg.max(1).values if am is None else xg.gather(1, am.long().unsqueeze(1)).squeeze(1)
    cat = torch.cat([x1, g1.repeat_interleave(N, 0)], 1)                          # tile + concat
    h = blocks(P, P2[:1], cat, N, False, eps, train, dec.get("concat0"))
    x2 = blocks(P, P2[1:], h, N, True, eps, train, dec.get("pointnet_2"))
    return cat, x2


def vfe_clas(P, x, train=True, dec=None, eps=1e-5, drop_p=0.7):
    """x [B, 3, N] float64 -> logits [B, num_classes]; classify/vfe/vfe.py:17-28"""
    dec = dec or {}
    _, x2 = features(P, x, train, dec, eps)
    return pointnet_ref.fc_block(P, "fc", x2, [0, 2, 5], dec.get("fc"), drop_p if train else 0.0)


def vfe_seg(P, x, train=True, dec=None, eps=1e-5):
    """x [B, 3, N] float64 -> logits [B, N, num_classes]; segment/vfe/vfe.py:25-39"""
    dec = dec or {}
    B, _, N = x.shape
    cat, x2 = features(P, x, train, dec, eps)
    rows = torch.cat([cat, x2.repeat_interleave(N, 0)], 1)                        # :34-35
    h = pointnet_ref.stack(P, "seg_net", [0], rows, N, False, eps, train, dec.get("seg0"))
    h = pointnet_ref.stack(P, "seg_net", [3, 6, 9], h, N, False, eps, train, dec.get("seg1"))
    w, b = P["seg_net.12.weight"].squeeze(-1), P["seg_net.12.bias"]
    return (h @ w.t() + b).reshape(B, N, -1)                                      # :36-37
