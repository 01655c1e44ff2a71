"""Float64 restatement of the T-Net PointNet classifier (/root/reference/PAPC/models/classify/pointnet/pointnet_Conv1D.py:4-104), for the
GPU tests of papc_amd.models.PointNet_Clas.  Plain torch on CPU tensors; autograd gives the reference gradients.

Parameters come as a dict of this package's state names (``mlp_1.0.weight`` ...) -> float64 tensors.  ``dec`` optionally pins the
discontinuous decisions to the kernels' own (see tests/torch_ref.stack_routed): per stack ``(argmax, alive, masks)``, per FC block
``(mask1, mask2, keep)`` -- the ReLU decisions of its two hidden layers and the dropout keep mask of the classifier."""
import torch

from tests import torch_ref


def _stack_params(P, name, idx):
    return [(P["%s.%d.weight" % (name, i)].squeeze(-1), P["%s.%d.bias" % (name, i)], P["%s.%d.weight" % (name, i + 1)],
             P["%s.%d.bias" % (name, i + 1)]) for i in idx]


def stack(P, name, idx, rows, N, pool, eps, train, dec=None, tally=None):
    """relu(bn(conv)) over the layers at ``idx`` of nn.Sequential ``name``; rows [B*N, Cin]; pool: max over each cloud's N rows.
    ``tally``: a dict that collects the pinned stacks' decision counts (torch_ref.stack_routed's stats, summed).  ``dec == "own"``: the chain's
    own decisions at this precision, appended to ``tally["own"]`` in call order (to measure a float32 run's drift from float64)."""
    params = _stack_params(P, name, idx)
    if train or dec is not None:
        # (eval with pinned decisions: the same routed chain on the running statistics -- the reference's own relu / max is fine for logits
        # and wrong for a gradient within rounding of a tie)
        running = None if train else [(P["%s.%d.running_mean" % (name, i + 1)], P["%s.%d.running_var" % (name, i + 1)]) for i in idx]
        if isinstance(dec, str):
            dec = torch_ref.own_decisions(rows.detach(), [tuple(a.detach() for a in q) for q in params], N if pool else 1, eps, running)
            tally.setdefault("own", []).append(dec)
        argmax, alive, masks = dec if dec is not None else (None, None, None)
        if pool:
            out, stats = torch_ref.stack_routed(rows, params, N, eps, argmax, alive, masks, running=running)
        else:
            # every row's activation: a max over groups of one row, pinned to the kernel's ReLU decisions when given
            C = params[-1][0].shape[0]
            am = torch.zeros(rows.shape[0], C, dtype=torch.long) if alive is not None else None
            out, stats = torch_ref.stack_routed(rows, params, 1, eps, am, alive, masks, running=running)
        if tally is not None:
            for k, v in stats.items():
                tally[k] = tally.get(k, 0) + v
            tally.setdefault("stacks", []).append((name, idx, stats))
        return out
    x = rows
    for l, (w, b, g, bt) in enumerate(params):           # eval: the running statistics normalise
        rm, rv = P["%s.%d.running_mean" % (name, idx[l] + 1)], P["%s.%d.running_var" % (name, idx[l] + 1)]
        x = torch.relu(((x @ w.t() + b) - rm) / torch.sqrt(rv + eps) * g + bt)
    return x.reshape(-1, N, x.shape[1]).max(1).values if pool else x


def fc_block(P, name, x, idx, dec=None, p=0.0, tally=None):
    """Linear - ReLU - Linear - ReLU - [Dropout(p)] - Linear of nn.Sequential ``name`` (layers at idx).  ``tally``: with pinned masks,
    ``tally["fc"]`` receives (name, pinned ReLU decisions that differ from the reference's own, decisions)"""
    m1, m2, keep = dec if dec is not None else (None, None, None)
    w = [P["%s.%d.weight" % (name, i)] for i in idx]
    b = [P["%s.%d.bias" % (name, i)] for i in idx]
    a1 = x @ w[0].t() + b[0]
    x1 = torch.where(m1, a1, torch.zeros_like(a1)) if m1 is not None else torch.relu(a1)
    a2 = x1 @ w[1].t() + b[1]
    x2 = torch.where(m2, a2, torch.zeros_like(a2)) if m2 is not None else torch.relu(a2)
    if tally is not None and m1 is not None and m2 is not None:
        flips = int((m1 != (a1.detach() > 0)).sum()) + int((m2 != (a2.detach() > 0)).sum())
        tally.setdefault("fc", []).append((name, flips, a1.numel() + a2.numel()))
    if keep is not None:
        x2 = torch.where(keep, x2 / (1.0 - p), torch.zeros_like(x2))
    return x2 @ w[2].t() + b[2]


def pointnet_clas(P, x, train=True, dec=None, eps=1e-5, drop_p=0.7, tally=None):
    """x [B, 3, N] float64 -> logits [B, num_classes]; pointnet_Conv1D.py:77-104 step by step"""
    dec = dec or {}
    B, _, N = x.shape
    pts0 = x.transpose(1, 2)                                                               # [B, N, 3]
    g = stack(P, "input_transform_net", [0, 3, 6], pts0.reshape(B * N, 3), N, True, eps, train, dec.get("input_transform_net"), tally)
    t = fc_block(P, "input_fc", g, [0, 2, 4], dec.get("input_fc"), tally=tally).reshape(B, 3, 3)        # :81-84
    pts = torch.bmm(pts0, t)                                                               # :86-88
    h = stack(P, "mlp_1", [0, 3], pts.reshape(B * N, 3), N, False, eps, train, dec.get("mlp_1"), tally)                  # :89
    g = stack(P, "feature_transform_net", [0, 3, 6], h, N, True, eps, train, dec.get("feature_transform_net"), tally)   # :91-92
    t = fc_block(P, "feature_fc", g, [0, 2, 4], dec.get("feature_fc"), tally=tally).reshape(B, 64, 64)  # :93-94
    h = torch.bmm(h.reshape(B, N, 64), t).reshape(B * N, 64)                              # :96-99
    f = stack(P, "mlp_2", [0, 3, 6], h, N, True, eps, train, dec.get("mlp_2"), tally)            # :100-101
    return fc_block(P, "fc", f, [0, 2, 5], dec.get("fc"), drop_p if train else 0.0, tally=tally)        # :102
