"""float64 restatement of the VoxNet classifier (PAPC/models/classify/voxnet/voxnet.py) for the tests, in two forms, torch on the CPU,
differentiable: ``literal`` is the source's op sequence (F.conv3d, batch statistics, leaky_relu, F.conv3d, max_pool3d, reshape, the head),
``closed`` the form the kernels implement (channel-last rows, tap-major K, 2x2x2 groups with member e = dz 4 + dy 2 + dx, flatten index
c Ep^3 + p).  P is {name: float64 tensor} under the model's parameter names (backbone.0 / .1 / .3, head.0 / .3).

Decisions: the pool winner, the two LeakyReLU signs and the dropout mask are decided by comparisons that fp32 rounding can flip on a near-tie
(or, the mask, by the kernel's hash).  ``dec = (win [B Ep^3, 32], sign of the normed y1 [B E1^3, 32] bool, sign of fc1's output [B, 128] bool,
keep [B, 128] or None)`` pins them, as tests/kdnet_ref.py takes ``dec``: the reference then routes every gradient the way the kernels did and
the comparison measures arithmetic, not routing.  Any entry may be None: the reference's own decision (first member on an exact tie, keep all).
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
SLOPE = 0.01
DROP_P = 0.2


def edges(E):
    e1 = (E - 5) // 2 + 1
    return e1, e1 - 2, (e1 - 2) // 2


def _stats(y, dims, stats):
    if stats is not None:
        return stats
    return y.mean(dims), y.var(dims, unbiased=False)


def literal(P, x, keep=None, stats=None):
    """voxnet.py:20-26 op by op.  x [B, 1, E, E, E]; keep [B, 128] (0/1) or None: the dropout mask (upscale in train); stats = (mean, var):
    the eval-mode norm -> (logits, {"flat", "mean", "var"})"""
    B = x.shape[0]
    y = F.conv3d(x, P["backbone.0.weight"], P["backbone.0.bias"], stride=2)
    mean, var = _stats(y, (0, 2, 3, 4), stats)
    v = lambda t: t.view(1, -1, 1, 1, 1)                                                          # noqa: E731
    a = F.leaky_relu((y - v(mean)) / torch.sqrt(v(var) + EPS) * v(P["backbone.1.weight"]) + v(P["backbone.1.bias"]), SLOPE)
    z = F.conv3d(a, P["backbone.3.weight"], P["backbone.3.bias"])
    flat = F.max_pool3d(z, 2, 2).reshape(B, -1)
    h = F.leaky_relu(flat @ P["head.0.weight"].t() + P["head.0.bias"], SLOPE)
    if keep is not None:
        h = h * keep.to(h.dtype) / (1.0 - DROP_P)
    return h @ P["head.3.weight"].t() + P["head.3.bias"], {"flat": flat, "mean": mean, "var": var}


def _patches(v, k, stride):
    """v [B, D, H, W, C] -> [B D' H' W', k^3 C], tap-major K: (tz, ty, tx, c)"""
    u = v.unfold(1, k, stride).unfold(2, k, stride).unfold(3, k, stride)                           # [B, D', H', W', C, k, k, k]
    u = u.permute(0, 1, 2, 3, 5, 6, 7, 4)
    return u.reshape(-1, k * k * k * v.shape[-1])


def backbone_closed(P, x, win=None, sign1=None, stats=None):
    """-> {"y1" [B E1^3, 32] pre-norm rows, "t" the norm's output (retains its gradient: the kernels' dz), "mean", "var", "flat" [B, 32 Ep^3],
    "win" uint8 [B Ep^3, 32], "sign1"}"""
    B, E = x.shape[0], x.shape[2]
    e1, e2, ep = edges(E)
    w1, w2 = P["backbone.0.weight"], P["backbone.3.weight"]
    y1 = _patches(x.reshape(B, E, E, E, 1), 5, 2) @ w1.reshape(32, 125).t() + P["backbone.0.bias"]
    mean, var = _stats(y1, 0, stats)
    t = (y1 - mean) / torch.sqrt(var + EPS) * P["backbone.1.weight"] + P["backbone.1.bias"]
    if t.requires_grad:
        t.retain_grad()
    s1 = (t.detach() > 0) if sign1 is None else sign1
    a = torch.where(s1, t, SLOPE * t)
    wk = w2.permute(0, 2, 3, 4, 1).reshape(32, 27 * 32)                                           # [co][tap][ci]
    z = _patches(a.view(B, e1, e1, e1, 32), 3, 1) @ wk.t() + P["backbone.3.bias"]                 # [B E2^3, 32]
    grp = z.view(B, ep, 2, ep, 2, ep, 2, 32).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(B * ep ** 3, 8, 32)      # member e = dz 4 + dy 2 + dx
    if win is None:
        d = grp.detach()
        best, win = d[:, 0].clone(), torch.zeros(d.shape[0], 32, dtype=torch.uint8)
        for e in range(1, 8):
            take = d[:, e] > best
            best = torch.where(take, d[:, e], best)
            win = torch.where(take, torch.full_like(win, e), win)
    pooled = torch.gather(grp, 1, win.long().view(-1, 1, 32)).view(B, ep ** 3, 32)
    flat = pooled.transpose(1, 2).reshape(B, 32 * ep ** 3)                                        # voxnet.py:23: index c Ep^3 + p
    return {"y1": y1, "t": t, "mean": mean, "var": var, "flat": flat, "win": win, "sign1": s1}


def closed(P, x, dec=None, stats=None):
    """the whole model in closed form -> (logits, the backbone's dict)"""
    win, sign1, sign2, keep = dec if dec is not None else (None, None, None, None)
    bb = backbone_closed(P, x, win, sign1, stats)
    h = bb["flat"] @ P["head.0.weight"].t() + P["head.0.bias"]
    s2 = (h.detach() > 0) if sign2 is None else sign2
    h = torch.where(s2, h, SLOPE * h)
    if keep is not None:
        h = h * keep.to(h.dtype) / (1.0 - DROP_P)
    return h @ P["head.3.weight"].t() + P["head.3.bias"], bb


def params(E, seed, num_classes=10):
    """float64 parameters under the model's names for an input edge E (head.0 takes 32 Ep^3 inputs): a negative and a tiny norm weight, a
    nonzero conv1 bias"""
    g = torch.Generator().manual_seed(seed)
    ep = edges(E)[2]
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)                             # noqa: E731
    gamma = 0.5 + torch.rand(32, generator=g, dtype=torch.float64)
    gamma[3] = -gamma[3]
    gamma[17] = 1e-3
    gamma[20] = -0.7
    return {"backbone.0.weight": rn(32, 1, 5, 5, 5) / np.sqrt(125.0), "backbone.0.bias": 0.3 * rn(32),
            "backbone.1.weight": gamma, "backbone.1.bias": 0.2 * rn(32),
            "backbone.3.weight": rn(32, 32, 3, 3, 3) / np.sqrt(864.0), "backbone.3.bias": 0.1 * rn(32),
            "head.0.weight": rn(128, 32 * ep ** 3) / np.sqrt(32.0 * ep ** 3), "head.0.bias": 0.1 * rn(128),
            "head.3.weight": rn(num_classes, 128) / np.sqrt(128.0), "head.3.bias": 0.1 * rn(num_classes)}


# ---- the occupancy grid --------------------------------------------------------------------------------------------------------------------

def occupancy_loop(points, edge=32):
    """PAPC/datasets/tools/build_VoxData.py:58-60 for every cloud of points [B, N, 3]: Python floats (the source parses text into them)"""
    h = (edge - 1) / 2.0
    out = np.zeros((len(points), 1, edge, edge, edge), np.float32)
    for b, cloud in enumerate(points):
        arr = np.zeros((edge,) * 3).astype('float32')
        for j in range(len(cloud)):
            arr[int(float(cloud[j][0]) * h + h)][int(float(cloud[j][1]) * h + h)][int(float(cloud[j][2]) * h + h)] = 1
        out[b, 0] = arr
    return out


def straddlers(edge=32, count=24):
    """float32 coordinates c in (-1, 1) whose index differs between a float32 and a float64 evaluation of c h + h: the values just below the
    coordinate at which the float64 value crosses an integer"""
    h32, h = np.float32((edge - 1) / 2.0), (edge - 1) / 2.0
    out = []
    for k in range(1, edge):
        c = np.float32((k - h) / h)
        for _ in range(4):
            c = np.nextafter(c, np.float32(-2.0))
            i64, i32 = int(float(c) * h + h), int(np.float32(c * h32 + h32))
            if i64 != i32:
                out.append(c)
                break
    return np.asarray(out[:count], np.float32)


def occupancy_fixture(edge=32, seed=3):
    """points [2, 96, 3] float32 inside [-1, 1]: random ones, the exact values -1, 0 and 1 on every axis, and straddlers()"""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.0, 1.0, size=(2, 96, 3)).astype(np.float32)
    pts[0, :3] = np.asarray([[-1.0, 0.0, 1.0], [1.0, -1.0, 0.0], [0.0, 1.0, -1.0]], np.float32)
    pts[1, 0] = np.asarray([1.0, 1.0, 1.0], np.float32)
    pts[1, 1] = np.asarray([-1.0, -1.0, -1.0], np.float32)
    s = straddlers(edge)
    n = min(len(s), 24)
    pts[0, 8:8 + n, 0] = s[:n]
    pts[1, 8:8 + n, 2] = s[:n]
    pts[1, 40:40 + n, 1] = s[:n]
    return pts
