"""float64 restatement of the KD-Net classifier (PAPC/models/classify/kdnet/kdnet.py) for the tests: one level, literally and in closed form,
and the whole model.  torch on the CPU, differentiable.

Decisions: a level's pair max and ReLU are decided by comparisons that fp32 rounding can flip on a near-tie.  ``dec = (win, alive)`` -- the
kernel's winner bytes [B*dim/2, F] and ``out > 0`` -- pins them, as tests/pointnet_seg_ref.py takes ``dec``: the reference then routes every
gradient along the rows the kernel chose, and the comparison measures arithmetic, not routing.
"""
import numpy as np
import torch

DIMS = (1024, 512, 256, 128, 64, 32, 16, 8, 4, 2)
WIDTHS = ((3, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 128))


def closed_form(sel, dim):
    """sel [..., dim] integers in 0..2 -> (k, p): pre-pool row n takes weight plane k = (3n + s) // dim at source point p = (3n + s) % dim"""
    j = 3 * np.arange(dim) + np.asarray(sel)
    return j // dim, j % dim


def level_literal(x, sel, w, b, dim):
    """kdnet.py:21-30 op by op.  x [B, Cin, dim], sel [dim] long (one vector for the batch, as the source has it), w [3F, Cin], b [3F]
    -> [B, F, dim/2]"""
    f = w.shape[0] // 3
    y = torch.relu(torch.einsum("oc,bcn->bon", w, x) + b.view(1, -1, 1))
    y = y.reshape(-1, f, 3, dim)
    y = y.reshape(-1, f, 3 * dim)
    y = torch.index_select(y, 2, sel + torch.arange(0, dim) * 3)
    y = y.reshape(-1, f, dim // 2, 2)
    return torch.max(y, dim=-1)[0]


def level(rows, sel, w, b, B, dim, dec=None):
    """The closed form on point-major rows.  rows [B*dim, Cin], sel [dim] or [B, dim] (integers), w [3F, Cin], b [3F] or None
    -> (out [B*dim/2, F], win uint8 [B*dim/2, F], alive bool): with dec = (win, alive) the kernel's decisions, else the reference's own
    (the first row of a pair on an exact tie)."""
    cin = rows.shape[1]
    f = w.shape[0] // 3
    s = torch.as_tensor(np.asarray(sel)).long()
    if s.dim() == 1:
        s = s.view(1, dim).expand(B, dim)
    j = 3 * torch.arange(dim).view(1, dim) + s
    k, p = j // dim, j % dim                                                           # [B, dim]
    xs = torch.gather(rows.view(B, dim, cin), 1, p.view(B, dim, 1).expand(B, dim, cin))
    y3 = xs @ w.t()                                                                    # [B, dim, 3F]: channel 3f + k
    if b is not None:
        y3 = y3 + b
    y = torch.gather(y3.view(B, dim, f, 3), 3, k.view(B, dim, 1, 1).expand(B, dim, f, 1)).view(B * dim // 2, 2, f)
    if dec is None:
        r = torch.relu(y.detach())
        win = (r[:, 1] > r[:, 0]).to(torch.uint8)
        alive = torch.maximum(r[:, 0], r[:, 1]) > 0
    else:
        win, alive = dec
    picked = torch.gather(y, 1, win.long().view(-1, 1, f)).view(-1, f)
    return torch.where(alive, picked, torch.zeros_like(picked)), win, alive


def kdnet(P, x, sels, dec=None):
    """P: {name: float64 tensor} (conv1 .. conv10 .weight [3F, Cin, 1] / .bias, fc.weight [classes, 128] / fc.bias), x [B, 3, 1024],
    sels: ten arrays [dim_l] or [B, dim_l], dec: ten (win, alive) or None -> logits [B, classes]"""
    B = x.shape[0]
    rows = x.transpose(1, 2).reshape(B * DIMS[0], 3)
    for i, dim in enumerate(DIMS):
        w = P["conv%d.weight" % (i + 1)]
        rows, _, _ = level(rows, sels[i], w.view(w.shape[0], -1), P["conv%d.bias" % (i + 1)], B, dim, None if dec is None else dec[i])
    return rows @ P["fc.weight"].t() + P["fc.bias"]


def fed_points(sel, B, dim):
    """bool [B, dim]: the source points that feed at least one pre-pool row (the others' input gradient is exactly zero)"""
    s = np.asarray(sel)
    if s.ndim == 1:
        s = np.broadcast_to(s, (B, dim))
    _, p = closed_form(s, dim)
    fed = np.zeros((B, dim), bool)
    np.put_along_axis(fed, p, True, 1)
    return fed
