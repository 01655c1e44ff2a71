"""torch-CPU transliteration of the reference's PointNet++ SSG classifier, in the reference's own op
decomposition -- TEST INFRASTRUCTURE / CPU BASELINE ONLY (see reference_np.py for the rules).

This is what ``bench.py``'s ``cpu_baseline`` leg times ("kind": "port"): PaddlePaddle cannot be installed on
either box, so the reference itself cannot run; this file keeps its *shape* -- the Python FPS loop with
host round-trips per iteration (pointnet2_basic_layers.py:79-93), the dense [B,S,N] distance matrix + int64
tile + full sort of query_ball_point (:110-124), numpy fancy-index gathers that cut autograd (:57-60), and
unfused Conv2d(1x1) / BatchNorm2d / relu / max (:215-219) -- with torch-CPU (MKL) standing in for paddle-CPU.
It doubles as a second opinion for the oracle: tests check its indices equal the C restatement bit for bit.
Run in double it is held at 1e-9 to the reference's own model code executed on the paddle stand-in (tests/test_reference_pin.py; see
reference_np.py).  Its norms are torch's: they put the UNBIASED batch variance into running_var where Paddle puts the biased one, which
nothing here reads (the pin tests redo that update the Paddle way).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as TF


def square_distance(src, dst):                                                   # :26-40
    B, N, _ = src.shape
    M = dst.shape[1]
    dist = -2 * torch.matmul(src, dst.transpose(1, 2))
    dist += torch.sum(src ** 2, -1).reshape(B, N, 1)
    dist += torch.sum(dst ** 2, -1).reshape(B, 1, M)
    return dist


def index_points(points, idx):                                                   # :43-62 (numpy round trip)
    B = points.shape[0]
    shape = list(idx.shape)
    view = [B] + [1] * (len(shape) - 1)
    rep = [1] + shape[1:]
    bidx = np.tile(np.arange(B).reshape(view), rep)
    return torch.from_numpy(points.detach().numpy()[bidx, idx.numpy().astype('int64'), :])


def farthest_point_sample(xyz, npoint, start_idx):                               # :65-95
    B, N, _ = xyz.shape
    centroids = torch.zeros(B, npoint)
    distance = torch.ones(B, N)
    farthest = torch.as_tensor(start_idx, dtype=torch.int64).clone()
    brange = np.arange(B)
    for i in range(npoint):
        centroids[:, i] = farthest
        centroid = torch.from_numpy(xyz.numpy()[brange, farthest.numpy(), :]).unsqueeze(1)
        dist = torch.sum((xyz - centroid) ** 2, -1)
        mask = (dist < distance).numpy()
        d_np, n_np = distance.numpy().copy(), dist.numpy()
        d_np[mask] = n_np[mask]
        distance = torch.from_numpy(d_np)
        farthest = torch.argmax(distance, -1)
    return centroids


def query_ball_point(radius, nsample, xyz, new_xyz):                             # :98-126
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    group_idx = torch.arange(N, dtype=torch.int64).reshape(1, 1, N).repeat(B, S, 1)
    sqrdists = square_distance(new_xyz, xyz)
    g = group_idx.numpy()
    g[(sqrdists > radius ** 2).numpy()] = N
    group_idx = torch.from_numpy(g).sort(dim=-1)[0][:, :, :nsample]
    first = group_idx[:, :, 0].reshape(B, S, 1).repeat(1, 1, nsample)
    g = group_idx.numpy().copy()
    m = g == N
    g[m] = first.numpy()[m]
    return torch.from_numpy(g)


def sample_and_group(npoint, radius, nsample, xyz, points, start_idx):           # :129-157
    B, N, C = xyz.shape
    fps_idx = farthest_point_sample(xyz, npoint, start_idx)
    new_xyz = index_points(xyz, fps_idx)
    idx = query_ball_point(radius, nsample, xyz, new_xyz)
    grouped = index_points(xyz, idx) - new_xyz.reshape(B, npoint, 1, C)
    if points is not None:
        grouped = torch.cat([grouped, index_points(points, idx)], dim=-1)
    return new_xyz, grouped, fps_idx, idx


class SetAbstraction(nn.Module):                                                 # :179-221
    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, group_all
        self.convs, self.bns = nn.ModuleList(), nn.ModuleList()
        last = in_channel
        for out in mlp:
            self.convs.append(nn.Conv2d(last, out, 1))
            self.bns.append(nn.BatchNorm2d(out))
            last = out

    def forward(self, xyz, points, start_idx=None):
        xyz = xyz.permute(0, 2, 1)
        if points is not None:
            points = points.permute(0, 2, 1)
        if self.group_all:
            B, N, C = xyz.shape
            new_xyz = torch.zeros(B, 1, C)
            new_points = xyz.reshape(B, 1, N, C)
            if points is not None:
                new_points = torch.cat([new_points, points.reshape(B, 1, N, -1)], dim=-1)
        else:
            new_xyz, new_points, _, _ = sample_and_group(self.npoint, self.radius, self.nsample, xyz.contiguous(),
                                                         None if points is None else points.contiguous(), start_idx)
        new_points = new_points.permute(0, 3, 2, 1)
        for conv, bn in zip(self.convs, self.bns):
            new_points = TF.relu(bn(conv(new_points)))
        new_points = torch.max(new_points, 2)[0]
        return new_xyz.permute(0, 2, 1), new_points


class FeaturePropagation(nn.Module):                                              # :284-335
    """Second opinion for reference_np.PointNetFeaturePropagation in the reference's own op decomposition
    (dense [B,N,S] distances, full sort, argsort OF THE SORTED matrix, fancy-index gather, Conv1d/BatchNorm1d)."""

    def __init__(self, in_channel, mlp):
        super().__init__()
        self.convs, self.bns = nn.ModuleList(), nn.ModuleList()
        last = in_channel
        for c in mlp:
            self.convs.append(nn.Conv1d(last, c, 1))
            self.bns.append(nn.BatchNorm1d(c, eps=1e-5))
            last = c

    def forward(self, xyz1, xyz2, points1, points2):
        xyz1, xyz2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2)
        points2 = points2.transpose(1, 2)
        B, N, _ = xyz1.shape
        S = xyz2.shape[1]
        if S == 1:
            interpolated = points2.repeat(1, N, 1)
        else:
            dists = square_distance(xyz1, xyz2)
            dists = torch.sort(dists, dim=-1).values                              # :316
            idx = torch.argsort(dists, dim=-1, stable=True)                        # :317
            dists, idx = dists[:, :, :3], idx[:, :, :3]
            dist_recip = 1.0 / (dists + 1e-8)
            norm = torch.sum(dist_recip, dim=2, keepdim=True)
            weight = dist_recip / norm
            interpolated = torch.sum(index_points(points2, idx) * weight.reshape(B, N, 3, 1), dim=2)
        if points1 is not None:
            new_points = torch.cat([points1.transpose(1, 2), interpolated], dim=-1)
        else:
            new_points = interpolated
        new_points = new_points.transpose(1, 2)
        for conv, bn in zip(self.convs, self.bns):
            new_points = TF.relu(bn(conv(new_points)))
        return new_points


class SSGClas(nn.Module):                       # classify/pointnet2/pointnet2.py:6-41
    def __init__(self, num_classes=16):
        super().__init__()
        self.sa1 = SetAbstraction(512, 0.2, 32, 3, [64, 64, 128], False)
        self.sa2 = SetAbstraction(128, 0.4, 64, 128 + 3, [128, 128, 256], False)
        self.sa3 = SetAbstraction(None, None, None, 256 + 3, [256, 512, 1024], True)
        self.fc1, self.bn1, self.drop1 = nn.Linear(1024, 512), nn.BatchNorm1d(512), nn.Dropout(0.4)
        self.fc2, self.bn2, self.drop2 = nn.Linear(512, 256), nn.BatchNorm1d(256), nn.Dropout(0.4)
        self.fc3 = nn.Linear(256, num_classes)

    def forward(self, xyz, start_idx=(None, None)):
        B = xyz.shape[0]
        l1_xyz, l1_points = self.sa1(xyz, None, start_idx[0])
        l2_xyz, l2_points = self.sa2(l1_xyz, l1_points, start_idx[1])
        _, l3_points = self.sa3(l2_xyz, l2_points)
        x = l3_points.reshape(B, 1024)
        x = self.drop1(TF.relu(self.bn1(self.fc1(x))))
        x = self.drop2(TF.relu(self.bn2(self.fc2(x))))
        return self.fc3(x)


def time_train_step(B, N, threads, seed=1234, repeats=1):
    """One fwd + CrossEntropy + bwd + Adam step (PAPC/train.py:106-116) on a seeded synthetic batch.
    Returns (seconds per step, clouds per second)."""
    import time
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from papc_amd.synthetic import make_clouds, make_labels, make_start_idx
    torch.set_num_threads(threads)
    torch.manual_seed(seed)
    model = SSGClas()
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-3)
    x = torch.from_numpy(make_clouds(B, N, seed))
    y = torch.from_numpy(make_labels(B, 16, seed)).reshape(-1)
    s1 = make_start_idx(B, N, seed)
    s2 = make_start_idx(B, 512, seed + 1)
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        loss = TF.cross_entropy(model(x, (s1, s2)), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, B / best


class SetAbstractionMsg(nn.Module):                                              # :224-281
    """PointNetSetAbstractionMsg in the reference's op decomposition: one FPS, then per radius a dense ball query, numpy gathers,
    in-place centre subtraction, concat [feats, xyz_norm] (feats first), Conv2d(1x1) / BatchNorm2d / relu, max over nsample."""

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint, self.radius_list, self.nsample_list = npoint, radius_list, nsample_list
        self.conv_blocks, self.bn_blocks = nn.ModuleList(), nn.ModuleList()
        for mlp in mlp_list:
            convs, bns = nn.ModuleList(), nn.ModuleList()
            last = in_channel + 3
            for out in mlp:
                convs.append(nn.Conv2d(last, out, 1))
                bns.append(nn.BatchNorm2d(out))
                last = out
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)

    def forward(self, xyz, points, start_idx=None):
        xyz = xyz.permute(0, 2, 1).contiguous()
        if points is not None:
            points = points.permute(0, 2, 1).contiguous()
        B, N, C = xyz.shape
        S = self.npoint
        new_xyz = index_points(xyz, farthest_point_sample(xyz, S, start_idx))
        outs = []
        for i, radius in enumerate(self.radius_list):
            K = self.nsample_list[i]
            group_idx = query_ball_point(radius, K, xyz, new_xyz)
            grouped_xyz = index_points(xyz, group_idx)
            grouped_xyz -= new_xyz.reshape(B, S, 1, C)
            if points is not None:
                grouped = torch.cat([index_points(points, group_idx), grouped_xyz], dim=-1)
            else:
                grouped = grouped_xyz
            grouped = grouped.permute(0, 3, 2, 1)
            for conv, bn in zip(self.conv_blocks[i], self.bn_blocks[i]):
                grouped = TF.relu(bn(conv(grouped)))
            outs.append(torch.max(grouped, 2)[0])
        return new_xyz.permute(0, 2, 1), torch.cat(outs, dim=1)


class MSGSeg(nn.Module):                        # segment/pointnet2/pointnet2.py:53-98
    def __init__(self, num_classes=16, num_parts=50):
        super().__init__()
        self.num_classes = num_classes
        self.sa1 = SetAbstractionMsg(512, [0.1, 0.2, 0.4], [32, 64, 128], 3, [[32, 32, 64], [64, 64, 128], [64, 96, 128]])
        self.sa2 = SetAbstractionMsg(128, [0.4, 0.8], [64, 128], 128 + 128 + 64, [[128, 128, 256], [128, 196, 256]])
        self.sa3 = SetAbstraction(None, None, None, 512 + 3, [256, 512, 1024], True)
        self.fp3 = FeaturePropagation(1536, [256, 256])
        self.fp2 = FeaturePropagation(576, [256, 128])
        self.fp1 = FeaturePropagation(150, [128, 128])
        self.conv1, self.bn1, self.drop1 = nn.Conv1d(128, 128, 1), nn.BatchNorm1d(128), nn.Dropout(0.5)
        self.conv2 = nn.Conv1d(128, num_parts, 1)

    def forward(self, xyz, cls_label, start_idx=(None, None)):
        B, C, N = xyz.shape
        l0_points, l0_xyz = xyz, xyz
        l1_xyz, l1_points = self.sa1(l0_xyz, l0_points, start_idx[0])
        l2_xyz, l2_points = self.sa2(l1_xyz, l1_points, start_idx[1])
        l3_xyz, l3_points = self.sa3(l2_xyz, l2_points)
        l2_points = self.fp3(l2_xyz, l3_xyz, l2_points, l3_points)
        l1_points = self.fp2(l1_xyz, l2_xyz, l1_points, l2_points)
        one_hot = TF.one_hot(cls_label.reshape(-1).long(), self.num_classes).float().reshape(B, self.num_classes, 1).repeat(1, 1, N)
        l0_points = self.fp1(l0_xyz, l1_xyz, torch.cat([one_hot, l0_xyz, l0_points], 1), l1_points)
        x = self.drop1(TF.relu(self.bn1(self.conv1(l0_points))))
        return self.conv2(x).permute(0, 2, 1)


class BasicClas(nn.Module):                     # classify/pointnet_base/pointnet_base.py:4-47
    def __init__(self, num_classes=16, max_points=1024):
        super().__init__()
        def blk(a, b):
            return [nn.Conv1d(a, b, 1), nn.BatchNorm1d(b), nn.ReLU()]
        self.mlp_1 = nn.Sequential(*blk(3, 64), *blk(64, 64))
        self.mlp_2 = nn.Sequential(*blk(64, 64), *blk(64, 128), *blk(128, max_points))
        self.fc = nn.Sequential(nn.Linear(1024, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Dropout(0.7), nn.Linear(256, num_classes))

    def forward(self, x):
        return self.fc(torch.max(self.mlp_2(self.mlp_1(x)), 2)[0])


class PFN(nn.Module):                            # detect/pointpillars/models/bones/pillars.py:9-108, one last PFNLayer (yaml num_filters [64])
    def __init__(self, vx=0.16, vy=0.16, pc_range=(0, -39.68, -3, 69.12, 39.68, 1)):
        super().__init__()
        self.linear = nn.Linear(9, 64, bias=False)
        self.norm = nn.BatchNorm1d(64, eps=1e-3, momentum=0.99)
        self.vx, self.vy, self.xo, self.yo = vx, vy, vx / 2 + pc_range[0], vy / 2 + pc_range[1]

    def forward(self, features, num_voxels, coors):
        mean = features[:, :, :3].sum(dim=1, keepdim=True) / num_voxels.to(features.dtype).reshape(-1, 1, 1)
        f_cluster = features[:, :, :3] - mean
        f_center = torch.zeros_like(features[:, :, :2])
        f_center[:, :, 0] = features[:, :, 0] - (coors[:, 3].float().unsqueeze(1) * self.vx + self.xo)
        f_center[:, :, 1] = features[:, :, 1] - (coors[:, 2].float().unsqueeze(1) * self.vy + self.yo)
        f = torch.cat([features, f_cluster, f_center], dim=-1)
        T = f.shape[1]
        mask = (num_voxels.unsqueeze(1) > torch.arange(T).reshape(1, -1)).unsqueeze(-1).to(f.dtype)
        f = f * mask
        x = self.linear(f)
        x = TF.relu(self.norm(x.permute(0, 2, 1)).permute(0, 2, 1))
        return torch.max(x, dim=1, keepdim=True)[0].squeeze()


def time_other_config(config, threads, seed=1234):
    """One fwd + loss + bwd + Adam step of another BASELINE config on the host cores -> (seconds, units, unit name, sample text)."""
    import os
    import sys
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from papc_amd.synthetic import make_clouds, make_pillars, make_start_idx
    torch.set_num_threads(threads)
    torch.manual_seed(seed)
    if config == "msg_seg":
        B, N = 16, 2048          # (the configuration's own batch: ~6 s per step on 64 cores, two or three steps inside the 20 s budget)
        model = MSGSeg().train()
        x = torch.from_numpy(make_clouds(B, N, 3))
        cls = torch.arange(B).reshape(B, 1) % 16
        tgt = torch.randint(0, 50, (B * N,))
        s1, s2 = make_start_idx(B, N, 3), make_start_idx(B, 512, 4)
        run = lambda: TF.cross_entropy(model(x, cls, (s1, s2)).reshape(B * N, 50), tgt)
        units, what = B, "B=%d N=%d PointNet2_MSG_Seg fwd+bwd+Adam" % (B, N)
    elif config == "basic":
        B, N = 8, 1024
        model = BasicClas().train()
        x = torch.from_numpy(make_clouds(B, N, 6))
        tgt = torch.randint(0, 16, (B,))
        run = lambda: TF.cross_entropy(model(x), tgt)
        units, what = B, "B=%d N=%d PointNet_Basic_Clas fwd+bwd+Adam" % (B, N)
    else:
        v, n, c = make_pillars()
        model = PFN().train()
        tv, tn, tc = torch.from_numpy(v), torch.from_numpy(n), torch.from_numpy(c)
        run = lambda: model(tv, tn, tc).square().mean()
        units, what = 1, "one 12000 x 100 frame, PillarFeatureNet fwd+bwd+Adam"
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-3)
    times = []
    while len(times) < 3 and (not times or sum(times) + times[-1] < 20.0):
        t0 = time.perf_counter()
        loss = run()
        opt.zero_grad()
        loss.backward()
        opt.step()
        times.append(time.perf_counter() - t0)
    t = sorted(times)[len(times) // 2]
    return t, units, what + ", median of %d step(s), %.2f s per step" % (len(times), t)
