"""The callers of the hot path, same constructors and forward contracts as the reference models.

  PointNet2_SSG_Clas / PointNet2_MSG_Clas  <- /root/reference/PAPC/models/classify/pointnet2/pointnet2.py:6-41, :43-75
  PointNet_Basic_Clas                      <- /root/reference/PAPC/models/classify/pointnet_base/pointnet_base.py:4-47
  PointNet_Clas (T-Net PointNet)           <- /root/reference/PAPC/models/classify/pointnet/pointnet_Conv1D.py:4-104
  PointNet2_SSG_Seg / PointNet2_MSG_Seg    <- /root/reference/PAPC/models/segment/pointnet2/pointnet2.py:6-52, :54-100
  PointNet_Seg (T-Net PointNet)            <- /root/reference/PAPC/models/segment/pointnet/pointnet.py:4-114
  PointNet_Basic_Seg                       <- /root/reference/PAPC/models/segment/pointnet_base/pointnet_base.py:4-80
  KDNet                                    <- PAPC/models/classify/kdnet/kdnet.py:5-49
  KDUNet                                   <- PAPC/models/segment/kdunet/kdunet.py:5-115
  VoxNet                                   <- PAPC/models/classify/voxnet/voxnet.py:4-26
  VFE_Clas / VFE_Seg                       <- PAPC/models/classify/vfe/vfe.py:5-86, PAPC/models/segment/vfe/vfe.py:5-97

Inputs are ``[B,3,N]`` float32 (``[B,6,N]`` with normals).  Everything runs in libpapc_hip.so, in train AND eval mode, the FC heads included
(head.py); the nn.Linear / BatchNorm1d / Dropout modules are the parameter holders.  CPU tensors raise PapcError (there is no CPU path); the
module chain remains only for TRAIN-mode head shapes outside the kernels' limits (more than 256 rows, widths that are no multiple of 4).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .layers import (PointNetFeaturePropagation, PointNetSetAbstraction, PointNetSetAbstractionMsg, _bn_buffers,
                     _stack_params)
from . import _lib
from . import head as _head
from .copyops import cat_copy
from .mlp import StackSpec, shared_mlp_max
from .plan import new_xyz

import os
_FUSED_HEAD = os.environ.get("PAPC_NO_FUSED_HEAD") != "1"     # A/B switch: fused classifier head (head.py) vs the library-op chain


def _starts(start_idx, n):
    if start_idx is None:
        return [None] * n
    assert len(start_idx) == n, "start_idx must hold one [B] tensor per FPS level"
    return list(start_idx)


def _bn1d(bn, y):
    """BatchNorm1d of the fallback head path with the convention of the fused kernels (and of paddle.nn.BatchNorm1D, which the
    reference uses: classify/pointnet2/pointnet2.py:18,21): in training the BIASED batch variance goes into the running estimate --
    torch's module would store the unbiased one, so the running statistics (and an exported .pdparams) would depend on which path a
    batch size selects."""
    if not (bn.training and bn.track_running_stats and y.shape[0] > 1):
        return bn(y)
    mean = y.mean(0)
    var = y.var(0, unbiased=False)
    mom = 0.1 if bn.momentum is None else float(bn.momentum)
    with torch.no_grad():
        bn.running_mean.mul_(1.0 - mom).add_(mean.detach(), alpha=mom)
        bn.running_var.mul_(1.0 - mom).add_(var.detach(), alpha=mom)
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked += 1
    return (y - mean) / torch.sqrt(var + bn.eps) * bn.weight + bn.bias


class _ClasHead:
    """fc1/bn1/drop1/fc2/bn2/drop2/fc3 (pointnet2.py:37-39): fused launches (head.py) in train and eval mode."""

    def _head(self, x, labels=None):
        """logits, or with ``labels`` (int64 [B]) the pair (mean softmax cross-entropy, logits): train.py:106-109's loss computed by the head's own
        launch (head.classifier_head_loss); the logits then carry no gradient."""
        spec = self.__dict__.get("_head_spec")
        if spec is None:
            spec = self.__dict__["_head_spec"] = _head.HeadSpec()
        if not x.is_cuda:
            raise _lib.PapcError("the classifier head needs CUDA (ROCm) tensors: there is no CPU fallback")
        if _FUSED_HEAD and _head.usable(x, self.fc1, self.fc2, self.fc3, self.training):
            if labels is not None:
                return _head.classifier_head_loss(spec, x, labels, self.fc1, self.bn1, self.drop1, self.fc2, self.bn2, self.drop2, self.fc3,
                                                  training=self.training)
            return _head.classifier_head(spec, x, self.fc1, self.bn1, self.drop1, self.fc2, self.bn2, self.drop2, self.fc3, training=self.training)
        # (train-mode shapes outside the kernels' limits, or PAPC_NO_FUSED_HEAD=1: the modules)
        x = self.drop1(F.relu(_bn1d(self.bn1, self.fc1(x))))
        x = self.drop2(F.relu(_bn1d(self.bn2, self.fc2(x))))
        logits = self.fc3(x)
        if labels is not None:
            return (_head.softmax_cross_entropy(logits, labels) if logits.is_cuda else F.cross_entropy(logits, labels.reshape(-1))), logits.detach()
        return logits


class PointNet2_SSG_Clas(nn.Module, _ClasHead):
    def __init__(self, name_scope='PointNet2_SSG_Clas_', num_classes=16, normal_channel=False, reference_quirks=False):
        super().__init__()
        in_channel = 6 if normal_channel else 3
        self.normal_channel = normal_channel
        q = dict(reference_quirks=reference_quirks)
        self.sa1 = PointNetSetAbstraction(npoint=512, radius=0.2, nsample=32, in_channel=in_channel, mlp=[64, 64, 128],
                                          group_all=False, **q)
        self.sa2 = PointNetSetAbstraction(npoint=128, radius=0.4, nsample=64, in_channel=128 + 3, mlp=[128, 128, 256],
                                          group_all=False, **q)
        self.sa3 = PointNetSetAbstraction(npoint=None, radius=None, nsample=None, in_channel=256 + 3,
                                          mlp=[256, 512, 1024], group_all=True, **q)
        self.fc1 = nn.Linear(1024, 512)
        self.bn1 = nn.BatchNorm1d(512)
        self.drop1 = nn.Dropout(0.4)
        self.fc2 = nn.Linear(512, 256)
        self.bn2 = nn.BatchNorm1d(256)
        self.drop2 = nn.Dropout(0.4)
        self.fc3 = nn.Linear(256, num_classes)

    def plan_sampling(self, inputs, start_idx=None, out=None, stage=None):
        """The whole weight-independent sampling pyramid of one batch (FPS1, ball query 1, FPS2, ball query 2): returns
        ((new_xyz1, idx1), (new_xyz2, idx2)).  Pass it to forward(plan=...); a training loop can compute it for batch
        i+1 on a side stream while batch i trains (see bench.py).  ``out`` = optional preallocated plan (same structure) that the
        kernels fill in place.  ``stage`` (needs ``out``): "fps1" = only the first level's farthest-point sampling, into out[0][0] (returns
        that tensor); "rest" = everything else, from the centroids out[0][0] already holds -- the two halves of a pyramid that a loop runs
        on two streams, the serial FPS chain one batch further ahead than the rest."""
        xyz = torch.as_tensor(inputs)
        if self.normal_channel:
            xyz = xyz[:, :3, :]
        s = _starts(start_idx, 2)
        with torch.no_grad():
            o = out if out is not None else (None, None)
            if stage == "fps1":
                return self.sa1.sample_fps(xyz, s[0], out=new_xyz(o[0]))
            p1 = self.sa1.sample(xyz, s[0], out=o[0], new_xyz=new_xyz(o[0]) if stage == "rest" else None)
            p2 = self.sa2.sample(new_xyz(p1).transpose(1, 2), s[1], out=o[1])
        return p1, p2

    def forward(self, inputs, start_idx=None, plan=None, after_sa2=None, tap=None, after_sa3=None, labels=None, after_sa1=None):
        """inputs [B,3,N]; ``labels`` = optional int64 [B]: return (loss, logits) instead of logits, the cross-entropy of train.py:106-109
        computed by the head's own launch; ``start_idx`` = optional (s1 [B], s2 [B]) FPS start indices (the source draws them at random);
        ``plan`` = optional result of :meth:`plan_sampling` for these inputs; ``after_sa2`` = optional callable invoked
        once SA2's kernels are enqueued -- from there to the end of SA3's backward only small-grid kernels run (group_all
        layer, FC head), the window in which a side stream can sample the next batch on otherwise idle CUs;
        ``tap`` = optional dict that receives ``l2_points``, the tensor SA3 consumes: a data-parallel loop runs the backward in
        two stages around it (head + SA3 first, their gradient bucket all-reducing while SA2 / SA1 follow; see bench.py)."""
        xyz = torch.as_tensor(inputs)
        B = xyz.shape[0]
        if self.normal_channel:
            norm, xyz = xyz[:, 3:, :], xyz[:, :3, :]
        else:
            norm = None
        s = _starts(start_idx, 2)
        pl = plan if plan is not None else (None, None)
        wt = None
        if torch.is_grad_enabled() and xyz.is_cuda:
            # the W^T operands of the three stacks' dX GEMMs in one launch (SA1 / SA2: layers 2, 3; SA3 also its first layer, whose
            # input features carry a gradient)
            from . import smallm
            from .mlp import precompute_wt
            ws = [c.weight for c in list(self.sa1.mlp_convs)[1:]] + [c.weight for c in self.sa2.mlp_convs]   # (SA2's first layer: the feature block of its W^T, gather-add backward)
            if not (smallm.takes_group_all(B, self.sa2.npoint, [c.weight.shape[0] for c in self.sa3.mlp_convs])):
                ws += [c.weight for c in self.sa3.mlp_convs]    # (the planes path builds its own W^T planes: nothing to transpose for it)
            # (SA2's gather-add first layer: its feature block, contiguous.  Lazy: SA1's forward reads nothing of the table, and where its first
            # layer runs through the coordinates' moments the transposes' launch carries that layer's finalize -- stack.SharedMLPStack)
            wt = precompute_wt(ws, feat_blocks=[(self.sa2.mlp_convs[0].weight, True)], lazy=True)
        l1_xyz, l1_points = self.sa1(xyz, norm, s[0], sampled=pl[0], wt_table=wt)
        if wt is not None:
            wt.flush()
        if after_sa1 is not None:
            after_sa1()
        l2_xyz, l2_points = self.sa2(l1_xyz, l1_points, s[1], sampled=pl[1], wt_table=wt)
        if after_sa2 is not None:
            after_sa2()
        if tap is not None:
            tap["l2_points"] = l2_points
        l3_xyz, l3_points = self.sa3(l2_xyz, l2_points, wt_table=wt)
        if after_sa3 is not None:
            after_sa3()
        x = l3_points.reshape(B, 1024)
        return self._head(x, labels)


class PointNet2_MSG_Clas(nn.Module, _ClasHead):
    def __init__(self, name_scope='PointNet2_MSG_Clas_', num_classes=16, normal_channel=False, reference_quirks=False):
        super().__init__()
        in_channel = 3 if normal_channel else 0
        self.normal_channel = normal_channel
        q = dict(reference_quirks=reference_quirks)
        self.sa1 = PointNetSetAbstractionMsg(512, [0.1, 0.2, 0.4], [16, 32, 128], in_channel,
                                             [[32, 32, 64], [64, 64, 128], [64, 96, 128]], **q)
        self.sa2 = PointNetSetAbstractionMsg(128, [0.2, 0.4, 0.8], [32, 64, 128], 320,
                                             [[64, 64, 128], [128, 128, 256], [128, 128, 256]], **q)
        self.sa3 = PointNetSetAbstraction(None, None, None, 640 + 3, [256, 512, 1024], True, **q)
        self.fc1 = nn.Linear(1024, 512)
        self.bn1 = nn.BatchNorm1d(512)
        self.drop1 = nn.Dropout(0.4)
        self.fc2 = nn.Linear(512, 256)
        self.bn2 = nn.BatchNorm1d(256)
        self.drop2 = nn.Dropout(0.5)
        self.fc3 = nn.Linear(256, num_classes)

    def forward(self, inputs, start_idx=None):
        xyz = torch.as_tensor(inputs)
        B = xyz.shape[0]
        if self.normal_channel:
            norm, xyz = xyz[:, 3:, :], xyz[:, :3, :]
        else:
            norm = None
        s = _starts(start_idx, 2)
        l1_xyz, l1_points = self.sa1(xyz, norm, s[0])
        l2_xyz, l2_points = self.sa2(l1_xyz, l1_points, s[1])
        l3_xyz, l3_points = self.sa3(l2_xyz, l2_points)
        x = l3_points.reshape(B, 1024)
        return self._head(x)


class PointNet_Basic_Clas(nn.Module):
    """Shared pointwise Conv1D+BN+ReLU stack (3->64->64->64->128->1024) -> max over N -> FC head.
    The five conv layers and the max are one SharedMLPMax node (group = one cloud, K = N)."""

    # checkpoint exchange: the source holds these layers in two nn.Sequential containers, mlp_1 = [conv, bn, relu] x 2 and
    # mlp_2 = [conv, bn, relu] x 3 (pointnet_base.py:7-25); papc_amd.checkpoint maps the names
    reference_names = {"convs.0": "mlp_1.0", "bns.0": "mlp_1.1", "convs.1": "mlp_1.3", "bns.1": "mlp_1.4", "convs.2": "mlp_2.0",
                       "bns.2": "mlp_2.1", "convs.3": "mlp_2.3", "bns.3": "mlp_2.4", "convs.4": "mlp_2.6", "bns.4": "mlp_2.7"}

    def __init__(self, num_classes=10, max_points=1024):
        super().__init__()
        chans = [3, 64, 64, 64, 128, max_points]
        self.convs = nn.ModuleList([nn.Conv1d(chans[i], chans[i + 1], 1) for i in range(5)])     # :8-24
        self.bns = nn.ModuleList([nn.BatchNorm1d(chans[i + 1], eps=1e-5) for i in range(5)])
        self.fc = nn.Sequential(nn.Linear(1024, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Dropout(p=0.7),
                                nn.Linear(256, num_classes))                                       # :26-33

    def forward(self, inputs):
        x = torch.as_tensor(inputs).float()                       # [B,3,N]
        B, _, N = x.shape
        xyz = x.transpose(1, 2)                                   # rows (b,n) read straight from the planar input
        zero = _lib.const_zeros((B, 1, 3), x.device)
        # the norms are registered layers in the source (nn.Sequential mlp_1 / mlp_2): model.eval() normalises with the running
        # statistics and leaves them untouched
        spec = StackSpec(B, N, 1, N, 0, xyz_first=True, eps=self.bns[0].eps, momentum=0.9, eval_bn=not self.training)
        ps = []
        for conv, bn in zip(self.convs, self.bns):
            ps += [conv.weight, conv.bias, bn.weight, bn.bias]
        feat = shared_mlp_max(spec, [(bn.running_mean, bn.running_var) for bn in self.bns], xyz, zero, None, None, ps)  # :42-44
        if _FUSED_HEAD and _head.plain_usable(feat, self.fc[0], self.fc[2], self.fc[5], self.training):
            spec = self.__dict__.get("_head_spec")
            if spec is None:
                spec = self.__dict__["_head_spec"] = _head.HeadSpec()
            return _head.plain_head(spec, feat, self.fc[0], self.fc[2], self.fc[4], self.fc[5], training=self.training)      # :26-33, :45 on the head kernels
        return self.fc(feat)                                      # :45


def _conv_bn_relu(chans, pool=None):
    """nn.Sequential([Conv1D, BatchNorm, ReLU] x len(chans) - 1 (+ MaxPool1D(pool))): the holders of one of pointnet_Conv1D.py's stacks, with
    the source's indices (conv 3i, norm 3i + 1)"""
    mods = []
    for i in range(len(chans) - 1):
        mods += [nn.Conv1d(chans[i], chans[i + 1], 1), nn.BatchNorm1d(chans[i + 1], eps=1e-5), nn.ReLU()]
    if pool is not None:
        mods.append(nn.MaxPool1d(pool))
    return nn.Sequential(*mods)


class PointNet_Clas(nn.Module):
    """PointNet with an input and a feature T-Net (/root/reference/PAPC/models/classify/pointnet/pointnet_Conv1D.py:4-104).

    The five Conv1D + BN + ReLU stacks run as shared-MLP nodes (one group per cloud, K = N; with the max over N where the source pools),
    the three T-Net / classifier FC blocks on the head kernels (transform.tnet_fc, head.plain_head), the two per-cloud matrix products
    x . T[b] on csrc/cloud_transform.hip (transform.py).  Containers and indices are the source's, so checkpoint.export_state /
    import_state exchange .pdparams with it directly.  The source pools with MaxPool1D(max_point): inputs must have N == max_point."""

    def __init__(self, num_classes=16, max_point=2048):
        super().__init__()
        self.max_point = int(max_point)
        self.input_transform_net = _conv_bn_relu([3, 64, 128, 1024], pool=max_point)                      # :7-18
        self.input_fc = nn.Sequential(nn.Linear(1024, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, 9))   # :19-28
        with torch.no_grad():
            self.input_fc[4].weight.zero_()                                                                  # :25 Assign(zeros)
            self.input_fc[4].bias.copy_(torch.eye(3).reshape(-1))                                            # :26 Assign(eye(3))
        self.mlp_1 = _conv_bn_relu([3, 64, 64])                                                              # :29-36
        self.feature_transform_net = _conv_bn_relu([64, 64, 128, 1024], pool=max_point)                     # :37-49
        self.feature_fc = nn.Sequential(nn.Linear(1024, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, 64 * 64))  # :50-56
        self.mlp_2 = _conv_bn_relu([64, 64, 128, 1024])                                                      # :57-66
        self.fc = nn.Sequential(nn.Linear(1024, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Dropout(p=0.7),
                                nn.Linear(256, num_classes))                                                 # :68-75

    def _spec(self, name):
        spec = self.__dict__.get(name)
        if spec is None:
            spec = self.__dict__[name] = _head.HeadSpec()
        return spec

    def _stack(self, seq, B, N, pool, xyz=None, zero=None, x_rows=None):
        """relu(bn(conv(.))) x layers of ``seq`` on the fused stack: from the planar coordinates (xyz) or from rows [B*N, C] (x_rows);
        pool: the max over each cloud's N rows -> [B, C_L], else every row -> [B*N, C_L].  The norms are registered layers of the source,
        so eval() normalises with their running statistics."""
        convs = [m for m in seq if isinstance(m, nn.Conv1d)]
        bns = [m for m in seq if isinstance(m, nn.BatchNorm1d)]
        spec = StackSpec(B, N, 1, N, 0, xyz_first=True, eps=bns[0].eps, momentum=0.9, pool=pool, eval_bn=not self.training)
        return shared_mlp_max(spec, _bn_buffers(bns), xyz, zero, None, None, _stack_params(convs, bns), x_rows=x_rows)

    def forward(self, inputs):
        x = torch.as_tensor(inputs).float()                                  # [B,3,N]
        if not x.is_cuda:
            raise _lib.PapcError("PointNet_Clas needs CUDA (ROCm) tensors: there is no CPU fallback")
        B, _, N = x.shape
        if N != self.max_point:
            raise _lib.PapcError("PointNet_Clas: the source pools with MaxPool1D(max_point): N = %d points per cloud, max_point = %d" % (N, self.max_point))
        from .transform import tnet_fc, transform_points, transform_rows
        g = self._stack(self.input_transform_net, B, N, True, xyz=x.transpose(1, 2), zero=_lib.const_zeros((B, 1, 3), x.device))   # :81-82
        t_in = tnet_fc(self._spec("_spec_input_fc"), g, self.input_fc).view(B, 3, 3)                   # :83-84
        pts = transform_points(x, t_in)                                                                # :86-88 -> [B, N, 3]
        h = self._stack(self.mlp_1, B, N, False, x_rows=pts.view(B * N, 3))                            # :89 -> [B*N, 64]
        g = self._stack(self.feature_transform_net, B, N, True, x_rows=h)                              # :91-92
        t_feat = tnet_fc(self._spec("_spec_feature_fc"), g, self.feature_fc).view(B, 64, 64)           # :93-94
        h = transform_rows(h, t_feat, N)                                                               # :96-99
        feat = self._stack(self.mlp_2, B, N, True, x_rows=h)                                           # :100-101 -> [B, 1024]
        if _FUSED_HEAD and _head.plain_usable(feat, self.fc[0], self.fc[2], self.fc[5], self.training):
            return _head.plain_head(self._spec("_head_spec"), feat, self.fc[0], self.fc[2], self.fc[4], self.fc[5], training=self.training)   # :102
        return self.fc(feat)                                                                           # :102


def _seg_net(cin, num_classes):
    """seg_net of both PointNet segmenters (segment/pointnet/pointnet.py:68-82, pointnet_base/pointnet_base.py:9-23): [Conv1D, BN, ReLU] x 4
    (cin -> 512 -> 256 -> 128 -> 128) and Conv1D(128, num_classes), at the source's indices 0..12"""
    return nn.Sequential(*(list(_conv_bn_relu([cin, 512, 256, 128, 128])) + [nn.Conv1d(128, num_classes, 1)]))


def _seg_input(model, inputs):
    """inputs[0] as the source takes it (the seg loader's [data, label] batch), or a bare [B, 3, N] tensor; a numpy array goes to the model's
    device (paddle.to_tensor), a CPU tensor raises PapcError"""
    import numpy as np
    if isinstance(inputs, (list, tuple)):
        inputs = inputs[0]
    if isinstance(inputs, np.ndarray):
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise _lib.PapcError("%s needs its parameters on a CUDA (ROCm) device: there is no CPU fallback" % type(model).__name__)
        inputs = torch.from_numpy(np.ascontiguousarray(inputs, dtype=np.float32)).to(dev)
    x = torch.as_tensor(inputs).float()
    if not x.is_cuda:
        raise _lib.PapcError("%s needs CUDA (ROCm) tensors: there is no CPU fallback" % type(model).__name__)
    return x


def _seg_head(model, point_rows, global_feat, B, N):
    """concat + seg_net (pointnet.py:105-114): seg_net[0..2] on segment.cloud_concat_bn_relu (the tile is never formed), [3..11] on one
    shared-MLP stack without the max, [12] on linear.linear_rows -> logits [B, N, num_classes]"""
    from .linear import linear_rows
    from .segment import cloud_concat_bn_relu
    s = model.seg_net
    h = cloud_concat_bn_relu(point_rows, global_feat, s[0], s[1], N, model.training)    # [B*N, 512]
    h = model._stack(list(s)[3:12], B, N, False, x_rows=h)                              # [B*N, 128]
    return linear_rows(h, s[12].weight, s[12].bias).view(B, N, -1)


class PointNet_Seg(nn.Module):
    """PointNet part segmentation with an input and a feature T-Net (/root/reference/PAPC/models/segment/pointnet/pointnet.py:4-114).

    The T-Nets, mlp_1 and the feature transform run as in PointNet_Clas; mlp_2 pools on the stack (the global feature); seg_net as _seg_head.
    Containers and indices are the source's, so checkpoint.export_state / import_state exchange .pdparams with it directly.  The source tiles
    the global feature by max_point: inputs must have N == max_point.  Output [B, N, num_classes]."""

    _spec = PointNet_Clas._spec
    _stack = PointNet_Clas._stack

    def __init__(self, num_classes=50, max_point=2048):
        super().__init__()
        self.max_point = int(max_point)
        self.input_transform_net = _conv_bn_relu([3, 64, 128, 1024], pool=max_point)                      # :8-20
        self.input_fc = nn.Sequential(nn.Linear(1024, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, 9))   # :21-30
        with torch.no_grad():
            self.input_fc[4].weight.zero_()                                                                  # :27 Assign(zeros)
            self.input_fc[4].bias.copy_(torch.eye(3).reshape(-1))                                            # :28 Assign(eye(3))
        self.mlp_1 = _conv_bn_relu([3, 64, 64])                                                              # :31-38
        self.feature_transform_net = _conv_bn_relu([64, 64, 128, 1024], pool=max_point)                     # :39-51
        self.feature_fc = nn.Sequential(nn.Linear(1024, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, 64 * 64))  # :52-58
        self.mlp_2 = _conv_bn_relu([64, 64, 128, 1024])                                                      # :59-68
        self.seg_net = _seg_net(1024 + 64, num_classes)                                                      # :69-83

    def forward(self, inputs):
        x = _seg_input(self, inputs)                                          # :85 inputs[0], [B,3,N]
        B, _, N = x.shape
        if N != self.max_point:
            raise _lib.PapcError("PointNet_Seg: the source tiles the global feature by max_point: N = %d points per cloud, max_point = %d" % (N, self.max_point))
        from .transform import tnet_fc, transform_points, transform_rows
        g = self._stack(self.input_transform_net, B, N, True, xyz=x.transpose(1, 2), zero=_lib.const_zeros((B, 1, 3), x.device))   # :88-89
        t_in = tnet_fc(self._spec("_spec_input_fc"), g, self.input_fc).view(B, 3, 3)                   # :90-91
        pts = transform_points(x, t_in)                                                                # :93-95 -> [B, N, 3]
        h = self._stack(self.mlp_1, B, N, False, x_rows=pts.view(B * N, 3))                            # :96 -> [B*N, 64]
        g = self._stack(self.feature_transform_net, B, N, True, x_rows=h)                              # :98-99
        t_feat = tnet_fc(self._spec("_spec_feature_fc"), g, self.feature_fc).view(B, 64, 64)           # :100-101
        point_feat = transform_rows(h, t_feat, N)                                                      # :103-107
        g = self._stack(self.mlp_2, B, N, True, x_rows=point_feat)                                     # :108-109 -> [B, 1024]
        return _seg_head(self, point_feat, g, B, N)                                                    # :110-114


class _PointNetBasicFeatures(nn.Module):
    """The source's PointNet_Basic of the segmenter (segment/pointnet_base/pointnet_base.py:41-76): the holders of mlp_1 / mlp_2"""

    def __init__(self, max_points=1024):
        super().__init__()
        self.mlp_1 = _conv_bn_relu([3, 64, 64])                          # :44-51
        self.mlp_2 = _conv_bn_relu([64, 64, 128, max_points])            # :52-62


class PointNet_Basic_Seg(nn.Module):
    """PointNet-Basic part segmentation (/root/reference/PAPC/models/segment/pointnet_base/pointnet_base.py:4-80): mlp_1 (per point) and
    mlp_2 pooled over each cloud (max_points channels) on the shared-MLP stack, then seg_net as PointNet_Seg's.  ``pointnet_bacic`` is the
    source's spelling, kept so that .pdparams load with no name table.  Inputs must have N == max_points.  Output [B, N, num_classes]."""

    _spec = PointNet_Clas._spec
    _stack = PointNet_Clas._stack

    def __init__(self, num_classes=50, max_points=1024):
        super().__init__()
        self.max_points = int(max_points)
        self.pointnet_bacic = _PointNetBasicFeatures(max_points)         # :7
        self.seg_net = _seg_net(max_points + 64, num_classes)            # :8-22

    def forward(self, inputs):
        x = _seg_input(self, inputs)                                     # :30 inputs[0], [B,3,N]
        B, _, N = x.shape
        if N != self.max_points:
            raise _lib.PapcError("PointNet_Basic_Seg: the source tiles the global feature by max_points: N = %d points per cloud, max_points = %d"
                                 % (N, self.max_points))
        from .copyops import contiguous_copy
        pts = contiguous_copy(x.transpose(1, 2)).view(B * N, 3)          # the planar coordinates as point rows
        h = self._stack(self.pointnet_bacic.mlp_1, B, N, False, x_rows=pts)   # :31 x1 -> [B*N, 64]
        g = self._stack(self.pointnet_bacic.mlp_2, B, N, True, x_rows=h)      # :31-32 max(x2) -> [B, max_points]
        return _seg_head(self, h, g, B, N)                               # :33-39


def Categorical(y, num_class=16):
    """pointnet2_basic_layers.py:7-14: class labels [B,1] (or [B]) -> one-hot float32 [B,num_class,1]."""
    y = torch.as_tensor(y).long().reshape(-1)
    # (a comparison instead of F.one_hot: that one reads min / max back to the host, which a hipGraph capture cannot contain)
    return (y.reshape(-1, 1) == torch.arange(num_class, device=y.device).reshape(1, -1)).to(torch.float32).unsqueeze(2)


class _PartSegBase(nn.Module):
    """Shared decoder half of the two part-segmentation nets (segment/pointnet2/pointnet2.py:36-51, :84-99): three
    feature-propagation levels, then conv1/bn1/relu/dropout/conv2 per point.  forward(inputs) with
    inputs = (points [B,C,N], cls_label [B,1]) -> logits [B,N,num_parts]."""

    def _head_init(self, num_parts):
        self.conv1 = nn.Conv1d(128, 128, 1)
        self.bn1 = nn.BatchNorm1d(128, eps=1e-5)
        self.drop1 = nn.Dropout(0.5)
        self.conv2 = nn.Conv1d(128, num_parts, 1)

    def _encode(self, l0_xyz, l0_points, start_idx, plan=(None, None, None, None)):
        raise NotImplementedError

    def sa1_first_weight(self):
        """first conv weight of the first set-abstraction level (SSG: mlp_convs, MSG: first radius branch)"""
        sa1 = self.sa1
        return (sa1.mlp_convs[0] if hasattr(sa1, "mlp_convs") else sa1.conv_blocks[0][0]).weight

    def plan_sampling(self, inputs, start_idx=None, out=None):
        """Everything of one batch that depends on the coordinates only: both sampling levels (FPS + ball queries, compact plans) and the
        3-NN searches of fp2 / fp1 -> (sa1 plan, sa2 plan, fp2 neighbours, fp1 neighbours).  Pass it to forward(plan=...); a training
        loop computes it for batch i + 1 on a side stream / graph branch while batch i trains (bench_configs.py).  ``out`` = a previous
        result for the same shapes that the kernels fill in place."""
        xyz = torch.as_tensor(inputs[0] if isinstance(inputs, (tuple, list)) else inputs)
        l0_xyz = xyz[:, :3, :] if self.normal_channel else xyz
        s = _starts(start_idx, 2)
        o = out if out is not None else (None, None, None, None)
        with torch.no_grad():
            p1 = self.sa1.sample(l0_xyz, s[0], out=o[0])
            l1_xyz = new_xyz(p1).transpose(1, 2)
            p2 = self.sa2.sample(l1_xyz, s[1], out=o[1])
            l2_xyz = new_xyz(p2).transpose(1, 2)
            n2 = self.fp2.plan(l1_xyz, l2_xyz, out=o[2])
            n1 = self.fp1.plan(l0_xyz, l1_xyz, out=o[3])
        return p1, p2, n2, n1

    def forward(self, inputs, start_idx=None, plan=None, after_encode=None):
        """``after_encode``: called once the three set-abstraction levels are enqueued, before the feature-propagation levels (a training
        loop forks the next batch's sampling branch here: the decoder's kernels are small and leave most of the chip idle)."""
        xyz = torch.as_tensor(inputs[0])
        dev = xyz.device
        cls_label = Categorical(inputs[1], self.num_classes).to(dev)                               # :28
        B, C, N = xyz.shape
        l0_points = xyz                                                                            # :32-37
        l0_xyz = xyz[:, :3, :] if self.normal_channel else xyz
        pl = plan if plan is not None else (None, None, None, None)
        (l1_xyz, l1_points), (l2_xyz, l2_points), (l3_xyz, l3_points) = self._encode(l0_xyz, l0_points, start_idx, pl)
        if after_encode is not None:
            after_encode()
        l2_points = self.fp3(l2_xyz, l3_xyz, l2_points, l3_points)                                 # :42
        l1_points = self.fp2(l1_xyz, l2_xyz, l1_points, l2_points, planned=pl[2])                  # :43
        cls_label_one_hot = cls_label.reshape(B, self.num_classes, 1).expand(B, self.num_classes, N)   # :44
        l0_points = self.fp1(l0_xyz, l1_xyz, cat_copy([cls_label_one_hot, l0_xyz.float(), l0_points.float()], 1), l1_points,
                             planned=pl[3])                                                        # :45
        rows = l0_points.transpose(1, 2).reshape(B * N, 128)            # point-major rows (a view of fp1's buffer)
        if not rows.is_cuda:
            raise _lib.PapcError("the segmentation head needs CUDA (ROCm) tensors: there is no CPU fallback")
        # :47 relu(bn1(conv1(.))) on the fused stack; eval: the running statistics normalise (bn1 IS registered in the source) and stay untouched
        spec = StackSpec(B, N, N, 1, 128, True, eps=self.bn1.eps, momentum=0.9, pool=False, eval_bn=not self.training)
        feat = shared_mlp_max(spec, _bn_buffers([self.bn1]), None, None, None, None,
                              _stack_params([self.conv1], [self.bn1]), x_rows=rows)
        x = self.drop1(feat)                                                                        # :48
        from .linear import linear_rows
        x = linear_rows(x, self.conv2.weight, self.conv2.bias)                                       # :49 (own row kernels, no library GEMM)
        return x.view(B, N, -1)                                                                     # :50 [B,N,num_parts]


class PointNet2_SSG_Seg(_PartSegBase):
    def __init__(self, name_scope='PointNet2_SSG_Seg_', num_classes=16, num_parts=50, normal_channel=False,
                 reference_quirks=False, fp_neighbours="reference"):
        super().__init__()
        additional_channel = 3 if normal_channel else 0
        self.num_classes, self.normal_channel = num_classes, normal_channel
        q = dict(reference_quirks=reference_quirks)
        self.sa1 = PointNetSetAbstraction(npoint=512, radius=0.2, nsample=32, in_channel=6 + additional_channel,
                                          mlp=[64, 64, 128], group_all=False, **q)
        self.sa2 = PointNetSetAbstraction(npoint=128, radius=0.4, nsample=64, in_channel=128 + 3, mlp=[128, 128, 256],
                                          group_all=False, **q)
        self.sa3 = PointNetSetAbstraction(npoint=None, radius=None, nsample=None, in_channel=256 + 3,
                                          mlp=[256, 512, 1024], group_all=True, **q)
        f = dict(neighbours=fp_neighbours, reference_quirks=reference_quirks)
        self.fp3 = PointNetFeaturePropagation(in_channel=1280, mlp=[256, 256], **f)
        self.fp2 = PointNetFeaturePropagation(in_channel=384, mlp=[256, 128], **f)
        self.fp1 = PointNetFeaturePropagation(in_channel=128 + 16 + 6 + additional_channel, mlp=[128, 128, 128], **f)
        self._head_init(num_parts)

    def _encode(self, l0_xyz, l0_points, start_idx, plan=(None, None, None, None)):
        s = _starts(start_idx, 2)
        l1 = self.sa1(l0_xyz, l0_points, s[0], sampled=plan[0])                                    # :38
        l2 = self.sa2(l1[0], l1[1], s[1], sampled=plan[1])                                         # :39
        l3 = self.sa3(l2[0], l2[1])                                                                # :40
        return l1, l2, l3


class PointNet2_MSG_Seg(_PartSegBase):
    def __init__(self, name_scope='PointNet2_MSG_Seg_', num_classes=16, num_parts=50, normal_channel=False,
                 reference_quirks=False, fp_neighbours="reference"):
        super().__init__()
        additional_channel = 3 if normal_channel else 0
        self.num_classes, self.normal_channel = num_classes, normal_channel
        q = dict(reference_quirks=reference_quirks)
        self.sa1 = PointNetSetAbstractionMsg(512, [0.1, 0.2, 0.4], [32, 64, 128], 3 + additional_channel,
                                             [[32, 32, 64], [64, 64, 128], [64, 96, 128]], **q)
        self.sa2 = PointNetSetAbstractionMsg(128, [0.4, 0.8], [64, 128], 128 + 128 + 64,
                                             [[128, 128, 256], [128, 196, 256]], **q)
        self.sa3 = PointNetSetAbstraction(npoint=None, radius=None, nsample=None, in_channel=512 + 3,
                                          mlp=[256, 512, 1024], group_all=True, **q)
        f = dict(neighbours=fp_neighbours, reference_quirks=reference_quirks)
        self.fp3 = PointNetFeaturePropagation(in_channel=1536, mlp=[256, 256], **f)
        self.fp2 = PointNetFeaturePropagation(in_channel=576, mlp=[256, 128], **f)
        self.fp1 = PointNetFeaturePropagation(in_channel=150 + additional_channel, mlp=[128, 128], **f)
        self._head_init(num_parts)

    def _encode(self, l0_xyz, l0_points, start_idx, plan=(None, None, None, None)):
        s = _starts(start_idx, 2)
        l1 = self.sa1(l0_xyz, l0_points, s[0], sampled=plan[0])                                    # :86
        l2 = self.sa2(l1[0], l1[1], s[1], sampled=plan[1])                                         # :87
        l3 = self.sa3(l2[0], l2[1])                                                                # :88
        return l1, l2, l3


class KDNet(nn.Module):
    """KD-Net classifier (PAPC/models/classify/kdnet/kdnet.py:5-49): ten levels of Conv1D(Cin, 3F, 1) + ReLU + kd-tree select + pair max
    (1024 points -> 1), then Linear(128, num_classes).  Every level is one kdnet.kdconv node (csrc/kdconv.hip: only the selected third of the
    conv is computed), the FC is linear.linear_rows.  Layer names and widths are the source's, so checkpoint.export_state / import_state
    exchange .pdparams with it directly.

    forward(inputs): inputs = [points, split_dims] as the source's loader yields them.  points [B, 3, 1024] (numpy or a device tensor);
    split_dims the source's list of ten arrays -- each [dim_l] (one cloud, or shared by the batch) or [B, dim_l], dim_l = 1024, 512, ... 2 --
    or one packed int32 tensor [2046] / [B, 2046] (kdnet.pack_split_dims; datasets.KDClasDataLoader yields the packed form).  -> [B, num_classes]"""

    WIDTHS = ((3, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 128))   # :8-17

    def __init__(self, name_scope='KDNet_', num_classes=10):
        super().__init__()
        for i, (cin, f) in enumerate(self.WIDTHS):
            setattr(self, "conv%d" % (i + 1), nn.Conv1d(cin, f * 3, 1, 1))
        self.fc = nn.Linear(128, num_classes)                                                    # :18

    def forward(self, inputs):
        import numpy as np
        from . import kdnet
        from .copyops import contiguous_copy
        from .linear import linear_rows
        points, split_dims = inputs[0], inputs[1]
        if isinstance(points, np.ndarray):                                                       # :31 paddle.to_tensor
            dev = next(self.parameters()).device
            if dev.type != "cuda":
                raise _lib.PapcError("KDNet needs its parameters on a CUDA (ROCm) device: there is no CPU fallback")
            points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
        x = torch.as_tensor(points).float()
        if not x.is_cuda or next(self.parameters()).device != x.device:
            raise _lib.PapcError("KDNet needs CUDA (ROCm) tensors and parameters on one device: there is no CPU fallback")
        if x.dim() != 3 or x.shape[1] != 3:
            raise _lib.PapcError("KDNet: points [B, 3, %d] expected, got %s" % (kdnet.DIMS[0], tuple(x.shape)))
        B, _, N = x.shape
        if N != kdnet.DIMS[0]:
            raise _lib.PapcError("KDNet: the source's ten levels halve %d points down to one: N = %d points per cloud, %d expected"
                                 % (kdnet.DIMS[0], N, kdnet.DIMS[0]))
        sel = kdnet.pack_split_dims(split_dims, B, x.device)
        rows = contiguous_copy(x.transpose(1, 2)).view(B * N, 3)                                 # the planar coordinates as point rows
        for i, dim in enumerate(kdnet.DIMS):                                                     # :35-44
            rows = kdnet.kdconv(rows, kdnet.level_split_dims(sel, i), getattr(self, "conv%d" % (i + 1)), B, dim)
        return linear_rows(rows, self.fc.weight, self.fc.bias)                                   # :45-46 ([B, 128, 1] -> [B, 128])


class _ConvBNReLU(nn.Module):
    """ConvBNReLU of kdunet.py:20-39: the holder of a 1x1 conv and its norm under the source's names"""

    def __init__(self, cin, cout):
        super().__init__()
        self._conv = nn.Conv1d(cin, cout, 1, 1)
        self._batch_norm = nn.BatchNorm1d(cout, eps=1e-5)


class _KDUNetDown(nn.Module):
    LEVELS = ((1024, 3, 32), (512, 32, 64), (256, 64, 256), (128, 256, 512), (64, 512, 1024))      # (dim, Cin, F), kdunet.py:44-48, :65-69

    def __init__(self):
        super().__init__()
        for i, (_, cin, f) in enumerate(self.LEVELS):
            setattr(self, "convbnrelu%d" % (i + 1), _ConvBNReLU(cin, f * 3))


class _KDUNetUp(nn.Module):
    WIDTHS = ((1024, 512, 1024, 512), (512, 512, 768, 512), (512, 256, 320, 256), (256, 256, 288, 128), (128, 128, 131, 128))   # kdunet.py:77-96

    def __init__(self, num_classes):
        super().__init__()
        for i, (cin, cup, ccat, cout) in enumerate(self.WIDTHS):
            setattr(self, "deconv%d" % (i + 1), nn.ConvTranspose1d(cin, cup, 2, 2))
            second = _ConvBNReLU(cout, cout) if i < 4 else nn.Conv1d(cout, num_classes, 1, 1)
            setattr(self, "doubleconv%d" % (i + 1), nn.Sequential(_ConvBNReLU(ccat, cout), second))


class KDUNet(nn.Module):
    """KDUNet part segmenter (PAPC/models/segment/kdunet/kdunet.py:5-115).  Down: five levels of Conv1D(Cin, 3F, 1) + BatchNorm + ReLU + kd-tree
    select + pair max (1024 points -> 32), each one kdnet.kdconv_bn node (csrc/kdbn.hip: only the selected third of the conv is computed, the
    BatchNorm statistics of all 3F channels come from the moments of the level's input rows).  Up: five times Conv1DTranspose(k = 2, s = 2) as a
    row GEMM (linear.linear_rows against the weight permuted to [2 Cout, Cin]: out[2i + t] = x[i] W[:, :, t] + bias), the concat with the level's
    input rows (deconv first), and the ConvBNReLU pair on the shared-MLP stack without the max; the closing Conv1D(128, num_classes) on
    linear_rows.  Module names and shapes are the source's, so checkpoint.export_state / import_state exchange .pdparams with it directly.

    forward(inputs): inputs = [points, split_dims].  points [B, 3, 1024] (numpy or a device tensor); split_dims as for KDNet (only the first
    five levels are read) or a list of just the first five arrays.  -> [B, 1024, num_classes]"""

    def __init__(self, num_classes=50):
        super().__init__()
        self.downsample = _KDUNetDown()
        self.upsample = _KDUNetUp(num_classes)

    @staticmethod
    def _pack5(split_dims, B, device):
        """a list of just the first five levels -> the packed form (the five levels KDUNet never reads are zeros)"""
        import numpy as np
        from . import kdnet
        items = split_dims if isinstance(split_dims, (list, tuple)) else [split_dims]
        if any((isinstance(v, torch.Tensor) and v.is_floating_point()) or (isinstance(v, np.ndarray) and v.dtype.kind not in "iu") for v in items):
            raise _lib.PapcError("KDUNet split dims: integer values (0, 1 or 2) expected, got a non-integer array")
        if isinstance(split_dims, (list, tuple)) and len(split_dims) == 5:
            per_cloud = any(getattr(v, "ndim", 1) == 2 for v in split_dims)
            if all(isinstance(v, torch.Tensor) and v.is_cuda for v in split_dims):
                rest = [torch.zeros((B, d) if per_cloud else (d,), dtype=torch.int32, device=device) for d in kdnet.DIMS[5:]]
            else:
                rest = [np.zeros((B, d) if per_cloud else (d,), np.int32) for d in kdnet.DIMS[5:]]
            split_dims = list(split_dims) + rest
        return kdnet.pack_split_dims(split_dims, B, device)

    def _cbr(self, blocks, B, N, x_rows):
        """relu(bn(conv(.))) x the ConvBNReLU blocks on the fused stack, every row kept: rows [B*N, C] -> [B*N, C_L]"""
        convs, bns = [m._conv for m in blocks], [m._batch_norm for m in blocks]
        spec = StackSpec(B, N, 1, N, 0, xyz_first=True, eps=bns[0].eps, momentum=0.9, pool=False, eval_bn=not self.training)
        return shared_mlp_max(spec, _bn_buffers(bns), None, None, None, None, _stack_params(convs, bns), x_rows=x_rows)

    def forward(self, inputs):
        import numpy as np
        from . import kdnet
        from .copyops import contiguous_copy
        from .linear import linear_rows
        points, split_dims = inputs[0], inputs[1]
        if isinstance(points, np.ndarray):                                                       # :12 paddle.to_tensor
            dev = next(self.parameters()).device
            if dev.type != "cuda":
                raise _lib.PapcError("KDUNet needs its parameters on a CUDA (ROCm) device: there is no CPU fallback")
            points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
        x = torch.as_tensor(points).float()
        if not x.is_cuda or next(self.parameters()).device != x.device:
            raise _lib.PapcError("KDUNet needs CUDA (ROCm) tensors and parameters on one device: there is no CPU fallback")
        if x.dim() != 3 or x.shape[1] != 3:
            raise _lib.PapcError("KDUNet: points [B, 3, %d] expected, got %s" % (kdnet.DIMS[0], tuple(x.shape)))
        B, _, N = x.shape
        if N != kdnet.DIMS[0]:
            raise _lib.PapcError("KDUNet: the source's five levels halve %d points down to 32: N = %d points per cloud, %d expected"
                                 % (kdnet.DIMS[0], N, kdnet.DIMS[0]))
        sel = self._pack5(split_dims, B, x.device)
        rows = contiguous_copy(x.transpose(1, 2)).view(B * N, 3)                                 # the planar coordinates as point rows
        shortcut = []
        for i, (dim, _, _) in enumerate(_KDUNetDown.LEVELS):                                     # :65-69
            shortcut.append(rows)
            blk = getattr(self.downsample, "convbnrelu%d" % (i + 1))
            rows = kdnet.kdconv_bn(rows, kdnet.level_split_dims(sel, i), blk._conv, blk._batch_norm, B, dim, self.training)
        up = self.upsample
        n = kdnet.DIMS[5]                                                                        # 32 points per cloud
        for i in range(5):                                                                       # :99-113
            dc, pair = getattr(up, "deconv%d" % (i + 1)), getattr(up, "doubleconv%d" % (i + 1))
            cin, cup = dc.weight.shape[0], dc.weight.shape[1]
            w2 = contiguous_copy(dc.weight.permute(2, 1, 0)).view(2 * cup, cin)                  # [Cin, Cout, 2] -> rows t * Cout + co
            rows = linear_rows(rows, w2, dc.bias.repeat(2) if dc.bias is not None else None).view(2 * B * n, cup)
            n *= 2
            rows = cat_copy([rows.unsqueeze(0), shortcut[4 - i].unsqueeze(0)], 2).squeeze(0)     # deconv first, then the level's input rows
            if i < 4:
                rows = self._cbr(list(pair), B, n, rows)
            else:
                rows = self._cbr([pair[0]], B, n, rows)
                rows = linear_rows(rows, pair[1].weight, pair[1].bias)
        return rows.view(B, N, -1)                                                               # :16 the final transpose: [B, N, classes]


class _VFEPointNet(nn.Module):
    """PointNet_Basic of vfe.py (classify :42-64, segment :53-75): mlp_1 = ConvBNReLU x 2, mlp_2 = ConvBNReLU x 3 under the source's names"""

    def __init__(self, cin, cout):
        super().__init__()
        self.mlp_1 = nn.Sequential(_ConvBNReLU(cin, 64), _ConvBNReLU(64, 64))
        self.mlp_2 = nn.Sequential(_ConvBNReLU(64, 64), _ConvBNReLU(64, 128), _ConvBNReLU(128, cout))

    def blocks(self):
        return list(self.mlp_1) + list(self.mlp_2)


class _VFE(nn.Module):
    """VFE of vfe.py (classify :66-86, segment :77-97): pointnet_1 per point, its max over the cloud tiled next to it, pointnet_2 pooled.
    pointnet_1 is one shared-MLP stack without the max, the max is pillars._GroupMax (x1 is post-ReLU), pointnet_2.mlp_1.0 runs on
    vfe.concat_k_bn_relu (the [B*N, 512] concat is never formed), the other four layers of pointnet_2 are one stack with the max."""

    def __init__(self, feature_channels=256, max_points=1024):
        super().__init__()
        self.max_points = int(max_points)
        self.pointnet_1 = _VFEPointNet(3, feature_channels)
        self.pointnet_2 = _VFEPointNet(feature_channels * 2, max_points)

    @staticmethod
    def _cbr(blocks, B, N, x_rows, pool, training):
        convs, bns = [m._conv for m in blocks], [m._batch_norm for m in blocks]
        spec = StackSpec(B, N, 1, N, 0, xyz_first=True, eps=bns[0].eps, momentum=0.9, pool=pool, eval_bn=not training)
        return shared_mlp_max(spec, _bn_buffers(bns), None, None, None, None, _stack_params(convs, bns), x_rows=x_rows)

    def features(self, x, training):
        """x [B, 3, N] -> (x1 [B*N, C], g1 = max_n x1 [B, C], x2 = max_n pointnet_2(concat) [B, max_points])"""
        from .copyops import contiguous_copy
        from .pillars import _GroupMax
        from .vfe import concat_k_bn_relu
        B, _, N = x.shape
        pts = contiguous_copy(x.transpose(1, 2)).view(B * N, 3)                  # the planar coordinates as point rows
        x1 = self._cbr(self.pointnet_1.blocks(), B, N, pts, False, training)     # x1 -> [B*N, C]
        g1 = _GroupMax.apply(x1, B, N)                                           # paddle.max(x1, axis=-1) -> [B, C]
        p2 = self.pointnet_2.blocks()
        h = concat_k_bn_relu(x1, g1, p2[0]._conv, p2[0]._batch_norm, N, training)    # tile + concat + mlp_1.0 -> [B*N, 64]
        x2 = self._cbr(p2[1:], B, N, h, True, training)                          # -> [B, max_points]
        return x1, g1, x2


class VFE_Clas(nn.Module):
    """VFE classifier (PAPC/models/classify/vfe/vfe.py:5-86): the VFE features pooled over each cloud, then the FC head of PointNet_Basic_Clas.
    Module names and shapes are the source's, so checkpoint.export_state / import_state exchange .pdparams with it directly.  The source tiles
    by max_points: inputs must have N == max_points.  forward(inputs [B, 3, N]) -> [B, num_classes]"""

    def __init__(self, num_classes=16, max_points=1024):
        super().__init__()
        self.max_points = int(max_points)
        self.vfe = _VFE(max_points=max_points)                                                              # :8
        self.fc = nn.Sequential(nn.Linear(max_points, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Dropout(p=0.7),
                                nn.Linear(256, num_classes))                                                # :9-16

    def forward(self, inputs):
        import numpy as np
        dev = next(self.parameters()).device
        if isinstance(inputs, np.ndarray) and dev.type == "cuda":                                           # :24 paddle.to_tensor of a loader batch
            inputs = torch.from_numpy(np.ascontiguousarray(inputs, dtype=np.float32)).to(dev)
        x = torch.as_tensor(inputs).float()
        if not x.is_cuda or dev != x.device:
            raise _lib.PapcError("VFE_Clas needs CUDA (ROCm) tensors and parameters on one device: there is no CPU fallback")
        if x.dim() != 3 or x.shape[1] != 3:
            raise _lib.PapcError("VFE_Clas: points [B, 3, %d] expected, got %s" % (self.max_points, tuple(x.shape)))
        if x.shape[2] != self.max_points:
            raise _lib.PapcError("VFE_Clas: the source tiles the cloud feature by max_points: N = %d points per cloud, max_points = %d"
                                 % (x.shape[2], self.max_points))
        _, _, feat = self.vfe.features(x, self.training)                                                    # :25, [B, max_points]
        if _FUSED_HEAD and _head.plain_usable(feat, self.fc[0], self.fc[2], self.fc[5], self.training):
            spec = self.__dict__.get("_head_spec")
            if spec is None:
                spec = self.__dict__["_head_spec"] = _head.HeadSpec()
            return _head.plain_head(spec, feat, self.fc[0], self.fc[2], self.fc[4], self.fc[5], training=self.training)   # :26 on the head kernels
        return self.fc(feat)                                                                                # :26


class VFE_Seg(nn.Module):
    """VFE part segmenter (PAPC/models/segment/vfe/vfe.py:5-97): seg_net over concat([x1, tile(max x1), tile(x2)]).  seg_net[0..2] runs on
    vfe.concat_k_bn_relu with the per-cloud vector [max x1 | x2], [3..11] on one shared-MLP stack without the max, [12] on linear.linear_rows.
    Module names and shapes are the source's.  Inputs must have N == max_points.  forward(inputs) takes the loader's [data, label] batch or a
    bare [B, 3, N] tensor -> [B, N, num_classes]"""

    _stack = PointNet_Clas._stack

    def __init__(self, feature_channels=256, num_classes=50, max_points=1024):
        super().__init__()
        self.max_points = int(max_points)
        self.vfe = _VFE(feature_channels, max_points)                                                       # :9
        self.seg_net = _seg_net(max_points + feature_channels * 2, num_classes)                             # :10-24

    def forward(self, inputs):
        from .linear import linear_rows
        from .vfe import concat_k_bn_relu
        x = _seg_input(self, inputs)                                                                        # :32 inputs[0], [B, 3, N]
        if next(self.parameters()).device != x.device:
            raise _lib.PapcError("VFE_Seg needs CUDA (ROCm) tensors and parameters on one device: there is no CPU fallback")
        if x.dim() != 3 or x.shape[1] != 3:
            raise _lib.PapcError("VFE_Seg: points [B, 3, %d] expected, got %s" % (self.max_points, tuple(x.shape)))
        B, _, N = x.shape
        if N != self.max_points:
            raise _lib.PapcError("VFE_Seg: the source tiles the cloud features by max_points: N = %d points per cloud, max_points = %d"
                                 % (N, self.max_points))
        x1, g1, x2 = self.vfe.features(x, self.training)                                                    # :33
        s = self.seg_net
        g = cat_copy([g1.unsqueeze(0), x2.unsqueeze(0)], 2).squeeze(0)                                      # the per-cloud half of :34-35, [B, C + P]
        h = concat_k_bn_relu(x1, g, s[0], s[1], N, self.training)                                           # :36 seg_net[0..2] -> [B*N, 512]
        h = self._stack(list(s)[3:12], B, N, False, x_rows=h)                                               # [B*N, 128]
        return linear_rows(h, s[12].weight, s[12].bias).view(B, N, -1)                                      # :36-37


class VoxNet(nn.Module):
    """VoxNet classifier (PAPC/models/classify/voxnet/voxnet.py:4-26): Conv3D(1, 32, 5, 2) + BatchNorm + LeakyReLU + Conv3D(32, 32, 3) + MaxPool3D(2)
    over a 32^3 occupancy grid, then Linear(6912, 128) + LeakyReLU + Dropout(0.2) + Linear(128, num_classes).  The backbone is one
    voxnet.voxconv_backbone node (csrc/voxconv.hip: implicit-GEMM convs, the norm on load, the pool in registers), both Linear layers are
    linear.linear_rows with voxnet.leaky_dropout between them.  The module tree is the source's (``backbone`` / ``head`` Sequentials), so the
    parameter names are ``backbone.0.weight`` ... ``head.3.bias`` and checkpoint.export_state / import_state exchange .pdparams with it directly.
    ``model.eval()``: the norm on its running statistics, no dropout, nothing updated.

    forward(inputs): the grid [B, 1, 32, 32, 32] float32 as the source's loader yields it (numpy) or a device tensor -> [B, num_classes]"""

    def __init__(self, name_scope='VoxNet_', num_classes=10):
        super().__init__()
        self.backbone = nn.Sequential(nn.Conv3d(1, 32, 5, 2), nn.BatchNorm3d(32), nn.LeakyReLU(), nn.Conv3d(32, 32, 3, 1), nn.MaxPool3d(2, 2, 0))     # :7-13
        self.head = nn.Sequential(nn.Linear(32 * 6 * 6 * 6, 128), nn.LeakyReLU(), nn.Dropout(0.2), nn.Linear(128, num_classes))                       # :14-19

    @property
    def head_spec(self):
        """the dropout's device rng state and mask export (head.HeadSpec), created on first use"""
        spec = self.__dict__.get("_head_spec")
        if spec is None:
            spec = self.__dict__["_head_spec"] = _head.HeadSpec()
        return spec

    def forward(self, inputs):
        import numpy as np
        from . import voxnet
        from .linear import linear_rows
        dev = next(self.parameters()).device
        if isinstance(inputs, np.ndarray):                                                       # :21 paddle.to_tensor
            if dev.type != "cuda":
                raise _lib.PapcError("VoxNet needs its parameters on a CUDA (ROCm) device: there is no CPU fallback")
            if inputs.dtype != np.float32:
                raise _lib.PapcError("VoxNet takes a float32 grid, got %s" % inputs.dtype)
            inputs = torch.from_numpy(np.ascontiguousarray(inputs)).to(dev)
        x = inputs
        if not isinstance(x, torch.Tensor) or not x.is_cuda or dev != x.device:
            raise _lib.PapcError("VoxNet needs CUDA (ROCm) tensors and parameters on one device: there is no CPU fallback")
        if x.dtype != torch.float32:
            raise _lib.PapcError("VoxNet takes a float32 grid, got %s" % x.dtype)
        if x.dim() != 5 or tuple(x.shape[1:]) != (1, voxnet.EDGE, voxnet.EDGE, voxnet.EDGE):
            raise _lib.PapcError("VoxNet: a grid [B, 1, %d, %d, %d] expected, got %s" % (voxnet.EDGE, voxnet.EDGE, voxnet.EDGE, tuple(x.shape)))
        b, h = self.backbone, self.head
        x = voxnet.voxconv_backbone(x, b[0], b[1], b[3], self.training)                          # :22-23 (flattened: [B, 6912])
        x = linear_rows(x, h[0].weight, h[0].bias)                                               # :15
        x = voxnet.leaky_dropout(self.head_spec, x, h[2].p, self.training)                       # :16-17
        return linear_rows(x, h[3].weight, h[3].bias)                                            # :18
