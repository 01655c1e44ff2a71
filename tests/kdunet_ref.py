"""float64 restatement of the KDUNet part segmenter (PAPC/models/segment/kdunet/kdunet.py) for the tests: one down level literally (op by op
on [B, C, dim] tensors) and on point-major rows, and the whole model.  torch on the CPU, differentiable: the BatchNorm statistics are
functions of the batch, so autograd of these forms carries the dense terms of the BatchNorm backward.

Decisions: a level's pair max and the ReLUs are decided by comparisons that fp32 rounding can flip on a near-tie.  ``dec = (win, alive)`` --
the kernel's winner bytes [B*dim/2, F] and ``out > 0`` -- pins a down level's, as tests/kdnet_ref.py takes ``dec``; ``up_dec`` pins the up
half's ReLU masks.  The reference then routes every gradient along the rows the kernel chose, and the comparison measures arithmetic.
"""
import numpy as np
import torch
import torch.nn.functional as F

LEVELS = ((1024, 3, 32), (512, 32, 64), (256, 64, 256), (128, 256, 512), (64, 512, 1024))       # (dim, Cin, F), kdunet.py:44-48, :65-69
EPS = 1e-5
MOMENTUM = 0.9                                                                                   # paddle.nn.BatchNorm: weighs the running value


def batch_norm(y, gamma, beta, axes, running=None, eps=EPS):
    """paddle.nn.BatchNorm over ``axes`` of y (the channel axis is the remaining one, axis 1 of [B, C, L] or of [M, C]).  Train mode
    (running is None): the biased batch statistics.  -> (normalised, mean, var)"""
    shape = [1] * y.dim()
    shape[1] = -1
    if running is None:
        mean = y.mean(axes)
        var = ((y - mean.view(shape)) ** 2).mean(axes)
    else:
        mean, var = running
    return (y - mean.view(shape)) / torch.sqrt(var.view(shape) + eps) * gamma.view(shape) + beta.view(shape), mean, var


def level_literal(x, sel, w, b, gamma, beta, dim, running=None):
    """kdunet.py:51-61 op by op.  x [B, Cin, dim], sel [dim] or [B, dim] long (the source's call once per cloud), w [3F, Cin], b [3F]
    -> (out [B, F, dim/2], mean [3F], var [3F])"""
    f = w.shape[0] // 3
    B = x.shape[0]
    y = torch.einsum("oc,bcn->bon", w, x) + b.view(1, -1, 1)                                      # :36
    y, mean, var = batch_norm(y, gamma, beta, (0, 2), running)                                    # :37
    y = torch.relu(y)                                                                             # :38
    y = y.reshape(-1, f, 3, dim)                                                                  # :54
    y = y.reshape(-1, f, 3 * dim)                                                                 # :55
    ar = torch.arange(0, dim) * 3
    s = torch.as_tensor(np.asarray(sel)).long()
    if s.dim() == 1:
        y = torch.index_select(y, 2, s + ar)                                                      # :56-57
    else:
        y = torch.stack([torch.index_select(y[i], 1, s[i] + ar) for i in range(B)])
    y = y.reshape(-1, f, dim // 2, 2)                                                             # :58
    return torch.max(y, dim=-1)[0], mean, var                                                     # :59


def _count(tally, key, n, of):
    if tally is not None:
        tally[key] = tally.get(key, 0) + int(n)
        tally["decisions"] = tally.get("decisions", 0) + int(of)


def level(rows, sel, w, b, gamma, beta, B, dim, dec=None, running=None, tally=None):
    """The same level on point-major rows, the norm over the full [B*dim, 3F] conv output.  rows [B*dim, Cin] -> (out [B*dim/2, F], win, alive,
    mean [3F], var [3F], zhat [B*dim/2, F] of the picked rows): with dec = (win, alive) the kernel's decisions, else the reference's own (the
    first row of a pair on an exact tie)."""
    f = w.shape[0] // 3
    s = torch.as_tensor(np.asarray(sel)).long()
    if s.dim() == 1:
        s = s.view(1, dim).expand(B, dim)
    j = 3 * torch.arange(dim).view(1, dim) + s
    k, p = j // dim, j % dim                                                                      # [B, dim]
    y3 = rows @ w.t()
    if b is not None:
        y3 = y3 + b
    a3, mean, var = batch_norm(y3, gamma, beta, (0,), running)                                    # [B*dim, 3F]: channel 3f + k
    z3 = (y3 - mean) / torch.sqrt(var + EPS)

    def pick(t):
        t = torch.gather(t.view(B, dim, 3 * f), 1, p.view(B, dim, 1).expand(B, dim, 3 * f))       # the source point's row
        return torch.gather(t.view(B, dim, f, 3), 3, k.view(B, dim, 1, 1).expand(B, dim, f, 1)).view(B * dim // 2, 2, f)
    y = pick(a3)
    r = torch.relu(y.detach())
    if dec is None:
        win = (r[:, 1] > r[:, 0]).to(torch.uint8)
        alive = torch.maximum(r[:, 0], r[:, 1]) > 0
    else:
        win, alive = dec
        # pinned decisions that differ from the reference's own: a winner strictly below its pair's max (an exact tie has two own winners), and
        # alive / dead of the pinned winner
        rw = torch.gather(r, 1, win.long().view(-1, 1, f)).view(-1, f)
        _count(tally, "winner_moves", (rw < torch.maximum(r[:, 0], r[:, 1])).sum(), rw.numel())
        _count(tally, "alive_flips", (alive != (torch.gather(y.detach(), 1, win.long().view(-1, 1, f)).view(-1, f) > 0)).sum(), rw.numel())
    idx = win.long().view(-1, 1, f)
    picked = torch.gather(y, 1, idx).view(-1, f)
    zhat = torch.gather(pick(z3), 1, idx).view(-1, f)
    return torch.where(alive, picked, torch.zeros_like(picked)), win, alive, mean, var, zhat


def _cbr(P, name, rows, mask, running, tally=None, export=None):
    """ConvBNReLU (kdunet.py:20-39) on rows [M, Cin]; mask: the kernel's ReLU decisions or None"""
    w = P[name + "._conv.weight"]
    y = rows @ w.view(w.shape[0], -1).t() + P[name + "._conv.bias"]
    run = None if running is None else (running[name + "._batch_norm.running_mean"], running[name + "._batch_norm.running_var"])
    y, mean, var = batch_norm(y, P[name + "._batch_norm.weight"], P[name + "._batch_norm.bias"], (0,), run)
    if export is not None:
        export.append(y.detach() > 0)
    if mask is not None:
        _count(tally, "relu_flips", (mask != (y.detach() > 0)).sum(), y.numel())
    return (torch.relu(y) if mask is None else torch.where(mask, y, torch.zeros_like(y))), mean, var


def kdunet(P, x, sels, dec=None, up_dec=None, running=None, tally=None, export=None):
    """P: {name: float64 tensor} under the model's parameter names, x [B, 3, 1024], sels: the first five split vectors ([dim_l] or [B, dim_l]),
    dec: five (win, alive) or None, up_dec: {(stack 1..5, layer 0..1): bool mask} (missing: the reference's own ReLU), running: None (train
    mode) or {buffer name: float64 tensor} (eval mode) -> (logits [B, 1024, classes], {norm module name: (batch mean, batch var)}).  ``tally``: a dict that counts the pinned decisions which
    differ from the reference's own (winner_moves, alive_flips, relu_flips, decisions); ``export``: a list that receives the reference's own
    decisions in call order -- five (win, alive), then the up half's ReLU masks"""
    B = x.shape[0]
    up_dec = up_dec or {}
    stats = {}
    rows = x.transpose(1, 2).reshape(B * LEVELS[0][0], 3)
    shortcut = []
    for i, (dim, _, _) in enumerate(LEVELS):
        n = "downsample.convbnrelu%d" % (i + 1)
        w = P[n + "._conv.weight"]
        shortcut.append(rows)
        run = None if running is None else (running[n + "._batch_norm.running_mean"], running[n + "._batch_norm.running_var"])
        rows, win, alive, mean, var, _ = level(rows, sels[i], w.view(w.shape[0], -1), P[n + "._conv.bias"], P[n + "._batch_norm.weight"],
                                               P[n + "._batch_norm.bias"], B, dim, None if dec is None else dec[i], run, tally)
        if export is not None:
            export.append((win, alive))
        stats[n + "._batch_norm"] = (mean, var)
    npts = LEVELS[-1][0] // 2
    for i in range(5):
        t = rows.view(B, npts, -1).transpose(1, 2)                                                # [B, C, L]
        t = F.conv_transpose1d(t, P["upsample.deconv%d.weight" % (i + 1)], P["upsample.deconv%d.bias" % (i + 1)], stride=2)     # :99 ...
        npts *= 2
        rows = torch.cat([t.transpose(1, 2).reshape(B * npts, -1), shortcut[4 - i]], 1)           # :100 concat along channels, deconv first
        n = "upsample.doubleconv%d" % (i + 1)
        rows, mean, var = _cbr(P, n + ".0", rows, up_dec.get((i + 1, 0)), running, tally, export)
        stats[n + ".0._batch_norm"] = (mean, var)
        if i < 4:
            rows, mean, var = _cbr(P, n + ".1", rows, up_dec.get((i + 1, 1)), running, tally, export)
            stats[n + ".1._batch_norm"] = (mean, var)
        else:
            w = P[n + ".1.weight"]
            rows = rows @ w.view(w.shape[0], -1).t() + P[n + ".1.bias"]
    return rows.view(B, LEVELS[0][0], -1), stats
