"""What the kd-level kernel tests of KD-Net (tests/test_gpu_kdnet.py) and KDUNet (tests/test_gpu_kdunet.py) share: the split vectors."""
import numpy as np


def _np(t):
    return t.detach().double().cpu().numpy()


def _split_vectors(B, dim, seed):
    """(name, sel) -- sel [dim] (shared by every cloud) or [B, dim]: shared, per cloud, all 0, all 2, and random ones whose rows at n = dim//3 and
    n = 2 dim//3 (where the weight plane changes) are set to each of 0, 1, 2"""
    rng = np.random.default_rng(seed)
    out = [("shared", rng.integers(0, 3, size=dim)), ("per cloud", rng.integers(0, 3, size=(B, dim))),
           ("all 0", np.zeros(dim, np.int64)), ("all 2", np.full((B, dim), 2))]
    for v in range(3):
        s = rng.integers(0, 3, size=(B, dim))
        s[:, dim // 3] = v
        s[:, (2 * dim) // 3] = v
        out.append(("boundary rows = %d" % v, s))
    return out
