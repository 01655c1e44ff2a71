"""The engineered groupings of tests/grouping_cases.py are what they claim (no GPU): counts per group, physical totals modulo 128, hub and
orphan membership, where the invalid slots sit -- through the numpy model of the compacted layout, so tests/test_gpu_groupings.py holds the
kernels to cases whose structure is checked on any machine."""
import numpy as np

from tests import grouping_cases as GC

G, S = GC.G, GC.S


def _flat(case):
    ii = case["idx"]
    assert ii.dtype == np.int32 and ii.shape == (GC.B, S, case["K"]) and (G * case["K"]) % 128 == 0
    return ii.reshape(G, case["K"])


def _true_multiplicities(ii, N):
    """{point: slots} per group; every out-of-range entry is the zero row, key -1"""
    out = []
    for row in ii:
        d = {}
        for p in row:
            k = int(p) if 0 <= p < N else -1
            d[k] = d.get(k, 0) + 1
        out.append(d)
    return out


def _model_multiplicities(ii, N):
    m = GC.plan_model(ii)
    rows = m["rows"]
    mult = GC.multiplicities(m["cidx"][:rows], m["wrow"][:rows], np.repeat(m["seg"], 8), len(ii))
    out = []
    for d in mult:
        e = {}
        for p, w in d.items():
            k = p if 0 <= p < N else -1
            e[k] = e.get(k, 0.0) + w
        out.append(e)
    return m, out


def _holds(case):
    """the compacted layout of the case carries every (group, point) with the multiplicity the padded lists give it"""
    ii = _flat(case)
    m, mult = _model_multiplicities(ii, case["N"])
    assert abs(float(m["wrow"].sum()) - G * case["K"]) < 0.5
    return m, mult == [{p: float(c) for p, c in d.items()} for d in _true_multiplicities(ii, case["N"])]


def test_generators_have_their_stated_structure():
    # E1: cnt 1, 8 rows per group, first-row weight 1 + K - 8 (the last group's also pays for the tail)
    for K in (8, 64):
        c = GC.e1_singletons(K)
        ii = _flat(c)
        m, ok = _holds(c)
        assert ok and (ii == ii[:, :1]).all() and (m["cnt"] == 1).all() and (m["c8"] == 8).all() and m["total"] == 8 * G == m["rows"]
        assert (m["wrow"][m["start"][:-1]] == 1 + K - 8).all() and (m["coef"] == K - 8).all()
    # E2: K distinct entries everywhere, nothing compacted, all weights 1
    c = GC.e2_full()
    ii = _flat(c)
    m, ok = _holds(c)
    assert ok and all(len(set(r)) == c["K"] for r in ii) and m["total"] == G * c["K"] and (m["wrow"] == 1).all() and not m["coef"].any()
    # E3: cnt = 1 + g mod K, copies at the tail only; 0 mod 8, 1 mod 8 and K all present
    for K in (16, 64):
        c = GC.e3_count_sweep(K)
        ii = _flat(c)
        m, ok = _holds(c)
        assert ok and c["K"] == K and m["cnt"].tolist() == [1 + g % K for g in range(G)]
        assert {8, 16} <= set(m["cnt"]) and {1, 9} <= set(m["cnt"]) and (K in m["cnt"] or K > G)      # (K = 64: 1 .. 32, no full group)
        for g in range(G):
            n = m["cnt"][g]
            assert len(set(ii[g, :n])) == n and (ii[g, n:] == ii[g, 0]).all()
    # E4: a -- total a multiple of 128, the last group without pad row or tail; b -- total = 8 mod 128, singleton last, 120-row tail
    m, ok = _holds(GC.e4_row_boundary("a"))
    assert ok and m["total"] % 128 == 0 and m["rows"] == m["total"] and m["cnt"][-1] % 8 == 0 and m["coef"][-1] == 16 - m["cnt"][-1]
    m, ok = _holds(GC.e4_row_boundary("b"))
    assert ok and m["total"] % 128 == 8 and m["rows"] - m["total"] == 120 and m["cnt"][-1] == 1
    assert m["coef"][-1] == 16 - 128 and m["wrow"][m["start"][-2]] == 1 + 16 - 128 and (m["seg"][m["start"][-2] // 8:] == G - 1).all()
    # E5: half the points orphans; the hub in every group -- a: never first, once; b: always first, with all the copies
    for v in ("a", "b"):
        c = GC.e5_hub_orphans(v)
        ii, N = _flat(c), c["N"]
        m, ok = _holds(c)
        assert ok and ii.max() < N // 2 and ii.min() >= 0                       # points N/2.. are in no group
        tm = _true_multiplicities(ii, N)
        if v == "a":
            assert all(d[GC.HUB] == 1 for d in tm) and (ii[:, 0] != GC.HUB).all()
        else:
            assert (ii[:, 0] == GC.HUB).all() and all(d[GC.HUB] == c["K"] - (m["cnt"][g] - 1) for g, d in enumerate(tm))
            assert min(d[GC.HUB] for d in tm) >= 2                              # every group has padding copies to carry
    # E6: a non-first index twice, the first index mid-list -- and the compacted layout LOSES a neighbour of the even groups (papc_hip.h,
    # papc_compact_plan_f32: copies of the first entry must sit at the tail), which is why E6 runs on the padded and list paths only
    c = GC.e6_interior_repeats()
    ii, N = _flat(c), c["N"]
    m, ok = _holds(c)
    assert not ok
    _, mult = _model_multiplicities(ii, N)
    tm = _true_multiplicities(ii, N)
    for g in range(G):
        first = ii[g, 0]
        mid = [k for k in range(1, c["K"]) if ii[g, k] == first and (ii[g, k + 1:] != first).any()]
        twice = [p for p, n in tm[g].items() if p != first and n == 2]
        assert len(mid) == 1 and len(twice) == 1
        lost = set(tm[g]) - set(mult[g])
        assert len(lost) == (1 if g % 2 == 0 else 0)
    # E7: N and -1 in non-first slots only (but for the all-N groups), both sentinels in both clouds, one all-N group per cloud
    for K, N in ((16, 64), (32, 64)):
        c = GC.e7_no_hit(K, N)
        ii = _flat(c)
        bad = (ii < 0) | (ii >= N)
        for g in range(G):
            if g in GC.ALL_N:
                assert (ii[g] == N).all()
            else:
                assert not bad[g, 0] and bad[g].sum() == (0, 1, 1, 2)[g % 4]
        assert sorted(GC.ALL_N)[0] < S <= sorted(GC.ALL_N)[1]
        for cl in range(GC.B):
            blk = ii[cl * S:(cl + 1) * S]
            assert (blk == N).any() and (blk == -1).any()
        _, ok = _holds(c)
        assert ok                                                                # (out-of-range entries are rows of their own: zero rows)
    # E8: the second half of the cloud repeats the first
    x = GC.e8_duplicated_cloud(128)
    assert x.shape == (GC.B, 3, 128) and np.array_equal(x[:, :, :64], x[:, :, 64:]) and len(np.unique(x[0, 0, :64])) == 64
    # the centres: the first neighbour's coordinates, finite also where the first slot is out of range
    c = GC.e7_no_hit()
    xyz, feats, new_xyz = GC.materialise(c, 16)
    assert feats.shape == (GC.B, c["N"], 16) and GC.materialise(c, 0)[1] is None
    for b in range(GC.B):
        for s in range(S):
            j = c["idx"][b, s, 0]
            if 0 <= j < c["N"]:
                assert np.array_equal(new_xyz[b, s], xyz[b, j])
            assert np.isfinite(new_xyz[b, s]).all()
