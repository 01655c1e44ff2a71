"""Engineered groupings for tests/test_gpu_groupings.py, and the numpy statement of the compacted layout they are checked against.

Every grouping in the rest of the suite is FPS + ball query on synthetic.make_clouds: about half the slots copies, always at the tail, no ball
empty of copies, no singleton, no point gathered by everything or by nothing.  The generators here build ``idx [B, S, K]`` int32 by hand so
that each structure stands alone.  numpy only: tests/test_groupings_host.py checks on any machine that the cases are what they claim."""
import numpy as np

B, S = 2, 16
G = B * S


def plan_model(ii):
    """The layout papc_compact_plan_f32 (csrc/compact.hip) makes of lists ii [G, K], as tests/test_gpu_compact.py::test_compact_plan_matches_numpy
    states it: cnt = 1 + #(k >= 1: ii[g, k] != ii[g, 0]); a group owns cnt rounded up to 8 rows -- the list's first rows BY POSITION, then copies
    of the first entry; the last group also takes the tail up to a multiple of 128; coef = K - rows of the group, wrow = 1 + coef on the first row."""
    ii = np.asarray(ii)
    Gn, K = ii.shape
    cnt = np.array([1 + int((row[1:] != row[0]).sum()) for row in ii])
    c8 = (cnt + 7) // 8 * 8
    start = np.concatenate([[0], np.cumsum(c8)]).astype(np.int64)
    total = int(start[-1])
    rows = (total + 127) // 128 * 128
    cidx = np.zeros(rows, np.int32)
    wrow = np.ones(rows, np.float32)
    seg = np.zeros(rows // 8, np.int32)
    coef = np.zeros(Gn, np.float32)
    for g in range(Gn):
        n = int(c8[g]) + (rows - total if g == Gn - 1 else 0)
        s0 = int(start[g])
        k = np.arange(n)
        cidx[s0:s0 + n] = np.where(k < c8[g], ii[g, np.minimum(k, K - 1)], ii[g, 0])
        coef[g] = K - n
        wrow[s0] = 1 + K - n
        seg[s0 // 8:(s0 + n) // 8] = g
    return dict(cnt=cnt, c8=c8, start=start, total=total, rows=rows, cidx=cidx, wrow=wrow, seg=seg, coef=coef)


def multiplicities(rows_pt, w, rows_grp, Gn):
    """{(group, point): summed weight} of a physical row layout -- what a layout claims the padded lists hold"""
    out = [dict() for _ in range(Gn)]
    for p, wt, g in zip(rows_pt, w, rows_grp):
        out[int(g)][int(p)] = out[int(g)].get(int(p), 0.0) + float(wt)
    return out


def _pad(distinct, K):
    d = [int(v) for v in distinct]
    return d + [d[0]] * (K - len(d))


def _from_counts(cnt, N, K, seed):
    rng = np.random.default_rng(seed)
    ii = np.zeros((G, K), np.int32)
    for g in range(G):
        ii[g] = _pad(rng.permutation(N)[:cnt[g]], K)
    return ii.reshape(B, S, K)


def e1_singletons(K):
    """every group K copies of one index: cnt = 1, 8 physical rows, first-row weight 1 + K - 8 (K = 8: nothing compacted, coef 0)"""
    N = 64
    ii = np.zeros((B, S, K), np.int32)
    for b in range(B):
        for s in range(S):
            ii[b, s, :] = (5 * s + 3 + 11 * b) % N
    return dict(name="E1 singletons K=%d" % K, N=N, K=K, idx=ii)


def e2_full(K=16):
    """every group K distinct indices: nothing is a copy, every weight 1, physical rows == padded rows"""
    N = 64
    return dict(name="E2 full", N=N, K=K, idx=_from_counts([K] * G, N, K, 2))


def e3_count_sweep(K=16):
    """group g has 1 + (g mod K) distinct neighbours: cnt = 0 mod 8 (no pad rows), 1 mod 8 (seven pad rows) and cnt = K in one grouping"""
    N = 96
    return dict(name="E3 count sweep", N=N, K=K, idx=_from_counts([1 + g % K for g in range(G)], N, K, 3))


def e4_row_boundary(variant, K=16):
    """'a': the physical total is exactly a multiple of 128 and the last group has a full multiple of 8 neighbours -- no pad row, no tail;
    'b': total = 8 mod 128 with a singleton last -- the last group carries a 120-row tail (its first-row weight is 1 + K - 128 < 0)"""
    N = 64
    cnt = [9 + g % 8 if g % 2 == 0 else 1 + g % 8 for g in range(G)]      # even groups 16 rows, odd groups 8: 384 = 3 * 128
    if variant == "b":
        cnt[1], cnt[G - 1] = 9, 1                                          # + 8 rows, singleton last: 392 = 3 * 128 + 8
    return dict(name="E4%s row boundary" % variant, N=N, K=K, idx=_from_counts(cnt, N, K, 4))


HUB = 5


def e5_hub_orphans(variant, K=16):
    """points N/2.. are gathered by no group; point HUB of each cloud is in EVERY group -- 'a': as a non-first neighbour (its list has S entries
    of weight 1), 'b': as every group's first neighbour (the padding multiplicity of every group lands on its entries)"""
    N = 64
    rng = np.random.default_rng(5)
    pool = np.array([p for p in range(N // 2) if p != HUB])
    ii = np.zeros((G, K), np.int32)
    for g in range(G):
        others = list(rng.permutation(pool)[:2 + g % 7])
        if variant == "a":
            others.insert(1 + g % len(others), HUB)
            ii[g] = _pad(others, K)
        else:
            ii[g] = _pad([HUB] + others, K)
    return dict(name="E5%s hub and orphans" % variant, N=N, K=K, idx=ii.reshape(B, S, K))


def e6_interior_repeats(K=16):
    """a non-first index twice and the first index again mid-list.  Even groups: [a b c b a d e f g | a x 7] -- seven non-first entries, so the
    compacted plan gives the group 8 rows, takes the list's first 8 positions and loses g (plan_model shows it); odd groups:
    [a b c d b e a f g h i | a x 5] -- sixteen rows, nothing lost"""
    N = 64
    rng = np.random.default_rng(6)
    ii = np.zeros((G, K), np.int32)
    for g in range(G):
        d = [int(v) for v in rng.permutation(N)[:11]]
        a = d[0]
        if g % 2 == 0:
            lst = [a, d[1], d[2], d[1], a, d[3], d[4], d[5], d[6]]
        else:
            lst = [a, d[1], d[2], d[3], d[1], d[4], a, d[5], d[6], d[7], d[8]]
        ii[g] = lst + [a] * (K - len(lst))
    return dict(name="E6 interior repeats", N=N, K=K, idx=ii.reshape(B, S, K))


ALL_N = (7, 20)      # the groups (one per cloud) that are entirely the no-hit sentinel


def e7_no_hit(K=16, N=64):
    """E3-like lists (3 + g mod (K - 2) entries, then copies of the first) with the no-hit sentinel N and -1 among the non-first entries AHEAD of
    the copies (g % 4 = 1: one N; 2: one -1; 3: a -1 at slot 1 and an N as the last entry), and one group per cloud that is entirely N"""
    cnt = [3 + g % (K - 2) for g in range(G)]
    ii = _from_counts(cnt, N, K, 7).reshape(G, K)
    for g in range(G):
        if g % 4 == 1:
            ii[g, 1 + g % (cnt[g] - 1)] = N
        elif g % 4 == 2:
            ii[g, 1 + (3 * g) % (cnt[g] - 1)] = -1
        elif g % 4 == 3:
            ii[g, 1], ii[g, cnt[g] - 1] = -1, N
    for g in ALL_N:
        ii[g, :] = N
    return dict(name="E7 no-hit rows K=%d" % K, N=N, K=K, idx=ii.reshape(B, S, K))


def materialise(case, D, seed=0):
    """seeded normal xyz [B, N, 3], feats [B, N, D] (None for D = 0) and new_xyz [B, S, 3] = the first neighbour's coordinates (a seeded normal
    centre where the first slot is out of range: such a row is a zero row whatever the centre)"""
    N, ii = case["N"], case["idx"]
    rng = np.random.default_rng(1000 + seed)
    xyz = rng.normal(size=(B, N, 3)).astype(np.float32)
    feats = rng.normal(size=(B, N, D)).astype(np.float32) if D else None
    new_xyz = rng.normal(size=(B, S, 3)).astype(np.float32)
    for b in range(B):
        for s in range(S):
            j = int(ii[b, s, 0])
            if 0 <= j < N:
                new_xyz[b, s] = xyz[b, j]
    return xyz, feats, new_xyz


def e8_duplicated_cloud(N=128, seed=8):
    """xyz [B, 3, N], points [B, D, N] whose second half of the points repeats the first (how real surfaces are padded to N)"""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-1, 1, size=(B, 3, N // 2))).astype(np.float32)
    return np.concatenate([x, x], axis=2)
