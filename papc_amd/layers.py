"""PointNet++ set-abstraction layers with the reference's constructor and forward signatures.

Mirrors /root/reference/PAPC/models/layers/pointnet2_basic_layers.py: ``PointNetSetAbstraction`` :179-221 and
``PointNetSetAbstractionMsg`` :224-281, ``PointNetFeaturePropagation`` :284-335.  forward(xyz [B,3,N], points [B,D,N] | None) -> (new_xyz [B,3,S],
new_points [B,D',S]).  The returned tensors are transposed *views* of point-major buffers ([B,S,3], [B,S,D']),
so chaining layers costs no transposes: the next layer's ``.transpose(1,2)`` (:203-205) is contiguous again.

Deliberate, flagged deviations from the source:
  * the conv/BN parameters are registered (``nn.ModuleList``) and trained; the source keeps them in plain Python
    lists (:185-191, :230-241) so its optimiser never sees them;
  * gradients flow through the gathers; the source cuts autograd at every ``index_points`` (:57-60).
  ``reference_quirks=True`` restores both behaviours (SA parameters frozen, gather gradients cut).
  * as in the source, the SA BatchNorms always normalise with batch statistics (``.eval()`` never reaches them).
"""
import os

import torch
import torch.nn as nn

from . import _lib
from . import functional as F_
from .compact import StackPolicy, point_lists
from .copyops import cat_copy, contiguous_copy, pad_cols
from .mlp import StackSpec, shared_mlp_max
from .plan import N_COMPACT, N_LISTS, N_XYZ_PRE, Cursor, Level


def _stack_params(convs, bns):
    ps = []
    for conv, bn in zip(convs, bns):
        ps += [conv.weight, conv.bias, bn.weight, bn.bias]
    return ps


def _bn_buffers(bns):
    return [(bn.running_mean, bn.running_var) for bn in bns]


def _pad_features(feats, params, xyz_first, feats_padded=None):
    """The gather kernels move features as float4: a feature count that is not a multiple of 4 (e.g. the 3 normal /
    xyz channels the segmentation nets feed to SA1) would fall to the element-wise path, ~10x slower.  Pad the features with
    zero channels and the first conv weight with matching zero columns instead (a view-level change: same result, the
    gradient flows back to the real columns through the concatenation)."""
    D = feats.shape[2] if feats_padded is None else feats_padded[1]
    pad = (-D) % 4
    if pad == 0:
        return feats, params, D
    if feats_padded is None:
        feats = pad_cols(feats, D, pad)
    else:
        feats = feats_padded[0]               # (padded once by the caller for several stacks: the MSG branches)
    w = params[0]
    w2 = w.reshape(w.shape[0], -1)
    # columns [xyz(3), feats(D)] -> [xyz, feats, 0]   or   [feats(D), xyz(3)] -> [feats, 0, xyz]
    w_pad = pad_cols(w2, w2.shape[1] if xyz_first else D, pad)
    return feats, [w_pad] + list(params[1:]), D + pad


class PointNetSetAbstraction(nn.Module):
    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all, reference_quirks=False, init_dist=1.0):
        super().__init__()
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last_channel, out_channel, 1))      # :189
            self.mlp_bns.append(nn.BatchNorm2d(out_channel, eps=1e-5))          # :190 (paddle default epsilon)
            last_channel = out_channel
        self.group_all = group_all
        self.reference_quirks = reference_quirks
        self.init_dist = init_dist   # the source initialises the FPS running distance with ones (:75)
        # compacted stack: None = decide once from the data, True / False = forced (compact.StackPolicy)
        self.compact = None
        self._policy = StackPolicy(self, self.mlp_convs, nsample, pad_width=False, padded_lists=True, keep_forced=False, never=group_all)
        if reference_quirks:
            for p in self.parameters():
                p.requires_grad_(False)

    @property
    def _compact_on(self):
        return self._policy.on

    def sample_fps(self, xyz, start_idx=None, out=None):
        """Farthest-point sampling alone (:143-144): xyz [B,3,N] -> new_xyz [B,S,3] (written into ``out`` when given).  The serial half of
        :meth:`sample` -- npoint dependent argmax steps on B workgroups -- which a training loop can run TWO batches ahead, beside the rest of
        the previous batch's pyramid (bench.py: the split pyramid)."""
        if self.group_all:
            return None
        xyz = xyz.transpose(1, 2)
        if xyz.dtype != torch.float32:
            xyz = xyz.float()
        return F_._fps_raw(xyz, self.npoint, start_idx, self.init_dist, new_xyz_out=out)[1]

    def sample(self, xyz, start_idx=None, out=None, new_xyz=None):
        """The weight-independent half of the layer (FPS + ball query, :143-145) on its own: xyz [B,3,N] ->
        (new_xyz [B,S,3], idx [B,S,K] int32, ...: the level's flat plan, plan.py).  Lets a training loop run batch i+1's sampling on a side
        stream while batch i's MLP kernels own the other CUs (FPS is a serial chain that occupies only B of the 256 CUs).
        ``out`` = optional previous result for the same shapes the kernels write straight into (no copies in a captured step);
        ``new_xyz`` = the centroids :meth:`sample_fps` already made for this xyz (no FPS here)."""
        if self.group_all:
            return None
        xyz = xyz.transpose(1, 2)
        if xyz.dtype != torch.float32:
            xyz = xyz.float()
        skip = _diag_skip(self.npoint) if out is not None else ()      # (timing diagnostics: stages left out, their buffers stale)
        w = Cursor(out)
        o_xyz, o_idx = w.next(2) or (None, None)
        if new_xyz is None:
            new_xyz = o_xyz if "fps" in skip else F_._fps_raw(xyz, self.npoint, start_idx, self.init_dist, new_xyz_out=o_xyz)[1]
        if "bq" in skip:
            idx = o_idx
        else:
            idx = F_._ball_query_raw([self.radius], [self.nsample], xyz, new_xyz, outs=None if o_idx is None else [o_idx])[0]
        w.put(new_xyz, idx)
        if self._xyz_first(xyz.shape[0]):
            # coordinates-only stack whose first layer runs through its input moments: the grouped centred coordinates and their
            # moments are weight-independent too (mlp.xyz_pregroup) -- part of the plan
            from .mlp import xyz_pregroup
            pre = w.next(N_XYZ_PRE)
            if "xyzpre" not in skip or pre is None:
                pre = xyz_pregroup(xyz, new_xyz, idx, out=pre)
            return w.put(*pre)
        # the compact plan and the grouping's point lists (the inverse index the gather-add backward sums over) are part of the plan too
        bufs = w.next(N_COMPACT, then=(0, N_LISTS))
        if "compact" in skip and bufs is not None:
            return tuple(out)
        cp = self._policy.plan(idx, out=bufs)
        if cp is not None:
            w.put(*cp.tensors())
        bufs = w.next(N_LISTS, then=(0,))
        if "lists" in skip and bufs is not None:
            return w.put(*bufs)
        if self._policy.wants_lists(cp is not None, xyz.shape[1]):
            w.put(*point_lists(xyz, new_xyz, idx, cp, out=bufs).tensors())
        return w.res

    def _xyz_first(self, B):
        from .mlp import xyz_first_layer_ok
        convs = self.mlp_convs
        return (not self.group_all and convs[0].in_channels == 3 and len(convs) >= 3
                and xyz_first_layer_ok(B * self.npoint * self.nsample, convs[0].out_channels, convs[1].out_channels, len(convs)))

    def forward(self, xyz, points, start_idx=None, sampled=None, wt_table=None):
        """xyz [B,3,N], points [B,D,N] or None -> new_xyz [B,3,S], new_points [B,D',S].
        ``sampled`` = optional (new_xyz, idx) from :meth:`sample` (skips FPS / ball query here);
        ``wt_table`` = optional result of ``mlp.precompute_wt`` covering this layer's weights, made for THIS forward pass."""
        xyz = xyz.transpose(1, 2)                                               # :203  [B,N,3] view
        if xyz.dtype != torch.float32:
            xyz = xyz.float()
        feats = None
        if points is not None:
            feats = contiguous_copy(points.float().transpose(1, 2))                 # :205  [B,N,D]
        B, N, _ = xyz.shape
        D = 0 if feats is None else feats.shape[2]
        if self.group_all:                                                      # sample_and_group_all :160-176
            S, K = 1, N
            new_xyz = _lib.const_zeros((B, 1, 3), xyz.device)                   # :170 (read-only: cached per device and batch size)
            idx = None
        else:                                                                   # sample_and_group :129-157
            S, K = self.npoint, self.nsample
            if sampled is not None:
                lv = Level.parse(sampled, B * S, [K])
            else:
                _, new_xyz = F_._fps_raw(xyz, S, start_idx, self.init_dist)
                lv = Level(new_xyz, F_._ball_query_raw([self.radius], [K], xyz, new_xyz))
                if feats is not None:
                    lv.cplans[0] = self._policy.plan(lv.idxs[0])
                    if self._policy.wants_lists(lv.cplans[0] is not None, N) and torch.is_grad_enabled():
                        lv.plists[0] = point_lists(xyz, new_xyz, lv.idxs[0], lv.cplans[0])
            new_xyz, idx = lv.new_xyz, lv.idxs[0]
        params = _stack_params(self.mlp_convs, self.mlp_bns)
        if feats is not None:
            feats, params, D = _pad_features(feats, params, True)
        spec = StackSpec(B, N, S, K, D, xyz_first=True, eps=self.mlp_bns[0].eps, momentum=0.9,
                         cut_gather_grad=self.reference_quirks)
        spec.wt_table = wt_table
        if not self.group_all and feats is None:
            spec.xyz_pre = lv.xyz_pre
        if not self.group_all and feats is not None:
            spec.compact, spec.plists = lv.cplans[0], lv.plists[0]
        out = shared_mlp_max(spec, _bn_buffers(self.mlp_bns), xyz, new_xyz, feats, idx, params)   # :214-219
        new_points = out.view(B, S, -1).transpose(1, 2)                         # [B,D',S]
        # (group_all: new_xyz is the cached READ-ONLY zero centre of sample_and_group_all, :170 -- a clone here would put a copy kernel
        # into every training step; callers must not edit the returned coordinates in place)
        return new_xyz.transpose(1, 2), new_points                              # :220-221


def _diag_skip(npoint):
    """PAPC_DIAG_SKIP=fps512,bq512,xyzpre512,fps128,bq128,compact128,lists128: stages of sample() to leave out when it writes into preallocated
    buffers (bench.py's sampling graph) -- what each stage costs the step; the plan is then STALE, results garbage.  Timing diagnostics only."""
    v = os.environ.get("PAPC_DIAG_SKIP")
    if not v:
        return ()
    suf = str(npoint)
    return tuple(t[:-len(suf)] for t in v.split(",") if t.endswith(suf))


MSG_BRANCH_STREAMS = os.environ.get("PAPC_MSG_STREAMS", "1") != "0"     # the MSG layers' radius branches on parallel streams
_BRANCH_STREAMS = {}


def set_branch_streams(model, on):
    """per-model switch for the MSG layers' parallel branch streams (None restores the process default); returns the previous settings"""
    old = []
    for m in model.modules():
        if isinstance(m, PointNetSetAbstractionMsg):
            old.append((m, m.branch_streams))
            m.branch_streams = on
    return old


def _branch_streams(dev, n):
    lst = _BRANCH_STREAMS.setdefault(str(dev), [])
    while len(lst) < n:
        lst.append(torch.cuda.Stream(device=dev))
    return lst[:n]


class PointNetSetAbstractionMsg(nn.Module):
    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list, reference_quirks=False, init_dist=1.0):
        super().__init__()
        self.npoint, self.radius_list, self.nsample_list = npoint, radius_list, nsample_list
        self.conv_blocks = nn.ModuleList()
        self.bn_blocks = nn.ModuleList()
        for i in range(len(mlp_list)):
            convs, bns = nn.ModuleList(), nn.ModuleList()
            last_channel = in_channel + 3                                       # :235
            for out_channel in mlp_list[i]:
                convs.append(nn.Conv2d(last_channel, out_channel, 1))
                bns.append(nn.BatchNorm2d(out_channel, eps=1e-5))
                last_channel = out_channel
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)
        self.reference_quirks = reference_quirks
        self.init_dist = init_dist
        self.compact = None            # compacted branches: None = decide once per branch from the data, True / False = forced (compact.StackPolicy)
        self._policies = [StackPolicy(self, convs, K, pad_width=True, padded_lists=False, keep_forced=True)
                          for convs, K in zip(self.conv_blocks, nsample_list)]
        self.branch_streams = None     # radius branches on parallel streams: None = the process default (PAPC_MSG_STREAMS), True / False = this layer
        if reference_quirks:
            for p in self.parameters():
                p.requires_grad_(False)

    @property
    def _compact_on(self):
        return {i: p.on for i, p in enumerate(self._policies) if p.on is not None}

    def sample(self, xyz, start_idx=None, out=None):
        """The weight-independent half (one FPS, one ball-query scan for all radii, :258-262) on its own: xyz [B,3,N] ->
        (new_xyz [B,S,3], idx_0 .. idx_{R-1} [B,S,K_r] int32, then per branch that runs compacted its compact-plan tensors and -- for a
        training layer -- the point-list tensors of that layout; plan.py has the layout).  ``out`` = a previous result of this method for the
        same shapes: the kernels write into it."""
        xyz = xyz.transpose(1, 2)
        if xyz.dtype != torch.float32:
            xyz = xyz.float()
        B, N, _ = xyz.shape
        w = Cursor(out)
        o = w.next(1 + len(self.radius_list))
        _, new_xyz = F_._fps_raw(xyz, self.npoint, start_idx, self.init_dist, new_xyz_out=None if o is None else o[0])
        idxs = F_._ball_query_raw(self.radius_list, self.nsample_list, xyz, new_xyz, outs=None if o is None else list(o[1:]))
        w.put(new_xyz, *idxs)
        for pol, idx in zip(self._policies, idxs):
            # (a branch that is still to be measured plans into fresh tensors: only a decided one knows that ``out`` holds its plan)
            cp = pol.plan(idx, out=w.next(N_COMPACT) if pol.mode(B) is True else None)
            if cp is not None:
                w.put(*cp.tensors())
                if pol.wants_lists(True, N):
                    w.put(*point_lists(xyz, new_xyz, idx, cp, out=w.next(N_LISTS)).tensors())
        return w.res

    def forward(self, xyz, points, start_idx=None, sampled=None):
        xyz = xyz.transpose(1, 2)                                               # :252
        if xyz.dtype != torch.float32:
            xyz = xyz.float()
        feats = None
        if points is not None:
            feats = contiguous_copy(points.float().transpose(1, 2))
        B, N, _ = xyz.shape
        D = 0 if feats is None else feats.shape[2]
        S = self.npoint
        R = len(self.radius_list)
        if sampled is not None:
            lv = Level.parse(sampled, B * S, self.nsample_list, compacted=[p.on is True and p.mode(B) is True for p in self._policies])
        else:
            _, new_xyz = F_._fps_raw(xyz, S, start_idx, self.init_dist)             # :258 (one FPS for all radii)
            lv = Level(new_xyz, F_._ball_query_raw(self.radius_list, self.nsample_list, xyz, new_xyz))   # :260-262, one scan
            if feats is not None:
                lv.cplans = [p.plan(idx) for p, idx in zip(self._policies, lv.idxs)]
                if torch.is_grad_enabled():
                    lv.plists = [point_lists(xyz, new_xyz, idx, cp) if (cp is not None and p.wants_lists(True, N)) else None
                                 for p, idx, cp in zip(self._policies, lv.idxs, lv.cplans)]
        new_xyz, idxs, cplans, plists = lv.new_xyz, lv.idxs, lv.cplans, lv.plists
        feats_in = feats
        padded = None
        if feats_in is not None and D % 4 != 0:          # (one padded copy of the features for all branches)
            padded = (pad_cols(feats_in, D, (-D) % 4), D)
        # The radius branches are independent until the concatenation (:264-280): branch i > 0 runs on its own stream (forked from / joined
        # into the caller's -- inside a hipGraph capture these become parallel graph branches), so one branch's launch-sized kernels
        # (BatchNorm finalizes, partial folds, the dependency gaps around them) run beside another branch's GEMMs.  Autograd replays each
        # branch's backward on the stream its forward ran on.
        par = (MSG_BRANCH_STREAMS if self.branch_streams is None else self.branch_streams) and xyz.is_cuda and R > 1
        side = _branch_streams(xyz.device, R - 1) if par else None
        main = torch.cuda.current_stream(xyz.device) if par else None

        def branch(i, K):
            params = _stack_params(self.conv_blocks[i], self.bn_blocks[i])
            Dp, feats_i = D, feats
            if feats_in is not None:
                feats_i, params, Dp = _pad_features(feats_in, params, False, padded)
            spec = StackSpec(B, N, S, K, Dp, xyz_first=False, eps=self.bn_blocks[i][0].eps, momentum=0.9,
                             cut_gather_grad=self.reference_quirks)             # feats first, then xyz (:267)
            if feats_in is not None:
                spec.compact = cplans[i]
                spec.plists = plists[i]
            o = shared_mlp_max(spec, _bn_buffers(self.bn_blocks[i]), xyz, new_xyz, feats_i, idxs[i], params)   # :271-276
            return o.view(B, S, -1)

        outs = [None] * R
        for i, K in enumerate(self.nsample_list):
            if par and i > 0:
                side[i - 1].wait_stream(main)
                # every tensor the branch reads was allocated on the caller's stream: tell the allocator the side stream uses it too, in the
                # forward here and in the backward autograd replays on the same stream (a freed block is otherwise handed to the next
                # main-stream allocation while a side-stream kernel may still be reading it)
                for t in (xyz, new_xyz, idxs[i], feats_in, None if padded is None else padded[0]) + lv.branch(i):
                    if t is not None:
                        t.record_stream(side[i - 1])
                with torch.cuda.stream(side[i - 1]):
                    outs[i] = branch(i, K)
                outs[i].record_stream(main)     # (consumed by the concatenation on the caller's stream)
            else:
                outs[i] = branch(i, K)
        if par:
            for s_ in side:
                main.wait_stream(s_)
        new_points_concat = cat_copy(outs, 2).transpose(1, 2)                   # :280  [B,D',S]
        return new_xyz.transpose(1, 2), new_points_concat


class PointNetFeaturePropagation(nn.Module):
    """:284-335.  forward(xyz1 [B,3,N], xyz2 [B,3,S], points1 [B,D1,N] | None, points2 [B,D2,S]) -> [B,D',N].

    ``neighbours``:
      * ``"reference"`` (default) -- what the source computes: it sorts ``dists`` and THEN argsorts the sorted
        matrix (:316-317), so its ``idx`` is 0,1,2 for every query: the three smallest distances weight the
        support points 0, 1 and 2.  Kept bit-compatible so a PAPC checkpoint / loss curve carries over.
      * ``"nearest"`` -- the PointNet++ paper's intent: the weights go to the three nearest support points.
    Same flagged deviations as the SA layers: parameters are registered and trained, and the gradient flows into
    ``points2`` through the interpolation (the source's ``index_points`` cuts it, :57-60);
    ``reference_quirks=True`` restores both.  The returned tensor is a transposed view of a point-major buffer.
    """

    def __init__(self, in_channel, mlp, neighbours="reference", reference_quirks=False):
        super().__init__()
        assert neighbours in ("reference", "nearest")
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv1d(last_channel, out_channel, 1))      # :291
            self.mlp_bns.append(nn.BatchNorm1d(out_channel, eps=1e-5))          # :292
            last_channel = out_channel
        self.neighbours = neighbours
        self.reference_quirks = reference_quirks
        if reference_quirks:
            for p in self.parameters():
                p.requires_grad_(False)

    def plan(self, xyz1, xyz2, out=None):
        """The weight-independent part of the layer -- the 3-NN search (:315-322) -- on its own: xyz1 [B,3,N], xyz2 [B,3,S] ->
        (dist3, idx3, w3) or None when S == 1.  A training loop can compute it with the sampling pyramid (models.*.plan_sampling)."""
        if xyz2.shape[2] == 1:
            return None
        return F_.three_nn(xyz1.transpose(1, 2), xyz2.transpose(1, 2), out=out)

    def interpolate(self, xyz1, xyz2, points2, planned=None):
        """:311-323 on point-major tensors: xyz1 [B,N,3], xyz2 [B,S,3], points2 [B,S,D] -> [B,N,D]"""
        B, N, _ = xyz1.shape
        S = xyz2.shape[1]
        if self.reference_quirks:
            points2 = points2.detach()
        if S == 1:
            return points2.expand(B, N, points2.shape[2])                        # paddle.tile (:312)
        _, idx3, w3 = planned if planned is not None else F_.three_nn(xyz1, xyz2)
        first3 = self.neighbours == "reference"
        if first3:
            idx3 = _lib.const_idx3(B, N, idx3.device)                                 # argsort of a sorted row: 0, 1, 2 (cached constant)
        return F_.three_interpolate(points2, idx3, w3, first3=first3)

    def forward(self, xyz1, xyz2, points1, points2, planned=None):
        xyz1 = xyz1.transpose(1, 2)                                              # :305-306
        xyz2 = xyz2.transpose(1, 2)
        points2 = points2.transpose(1, 2)                                        # :308
        B, N, _ = xyz1.shape
        interpolated = self.interpolate(xyz1, xyz2, points2, planned)
        if points1 is not None:
            new_points = cat_copy([points1.transpose(1, 2).float(), interpolated], 2)         # :326-327
        else:
            new_points = interpolated
        rows = new_points.reshape(B * N, new_points.shape[2])
        if not rows.is_contiguous():
            rows = rows.contiguous()
        spec = StackSpec(B, N, N, 1, rows.shape[1], True, eps=self.mlp_bns[0].eps, momentum=0.9, pool=False)
        out = shared_mlp_max(spec, _bn_buffers(self.mlp_bns), None, None, None, None,
                             _stack_params(self.mlp_convs, self.mlp_bns), x_rows=rows)   # :331-333
        return out.view(B, N, -1).transpose(1, 2)
