"""The voxconv and kd-level backward product loops held to the EXACT fp32 product, bit for bit: the sibling of tests/test_gpu_exact_products.py.

That file's docstring has the method (three-plane probe pairs, single terms and <= 8 equal terms, the int32 comparison, no tolerance), the table
of all product loops with the case that reaches each, the measured record and the account of what a broken loop does to both files.  Here are
the cases of the six loaders that reach vox_step / mfma_bf16x3 through operand selection of their own:

  papc_voxconv2_prep_f32       wk / wt are the two NumPy transposes of w2, bit for bit (every conv2 case below reads them from the device)
  papc_voxconv2_pool_fwd_f32   y1 zero but for a period-3 lattice per axis, ONE positive channel per lattice point: a 3-wide window holds exactly
                               one lattice point, so every pre-pool element is one term y1[pos, ci] W2[co, ci, tap]; W2 positive with the
                               exponent +-4 (tz - 1) +- 2 (ty - 1) +- (tx - 1) + ci % 3 - 1, signs from three bits of co: injective on the 2x2x2 cube
                               of taps through which a group's eight members see one lattice point, so the pooled maximum is strict
  papc_voxconv2_bwd_dx_f32     gout non-zero in ONE channel of the pool groups on a period-2 lattice of group coordinates: a y1 row's 27 pre-pool
                               positions span two adjacent groups per axis, one of them live -- dz is one term gout W2[co, ci, tap] or an exact
                               zero; y1 < 0 on a known subset pins the LeakyReLU' gate (fl32(0.01 acc), one rounding)
  papc_voxconv2_bwd_dw_f32     y1 dense, positive, identical in every cloud; channel co has its gradient at one (group, winner) in 4, 2 or 1 clouds:
                               27 648 sums of 4, 2, 1 equal terms folded over two chunks of 64 groups, db2 = n v
  papc_voxconv1_bwd_dw_f32     x dense and identical in every cloud, dz in one row per cloud: dW1 is 4, 2, 1 equal terms over four row chunks, db1 the
                               exact 0
  papc_kdconv_bwd_f32, dX      gout in one feature per pooled row, the winner parity chosen greedily so that no source point is fed by two live
                               rows; decoys with out = 0, and every live element seen with the OTHER parity from its pair's second row
  papc_kdconv_bwd_f32, dW, db  per plane classes of 4, 2, 1 pooled rows with identical x rows, over a full chunk of 128 rows and a ragged one of 72

test_every_loader_case (NumPy, runs everywhere) verifies every operand set with Probe.verify() and asserts the conditions a case leans on: the
share of strict maxima, the shares of non-zero rows, the coverage of taps, channels, members and planes.
"""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib
from tests.test_gpu_exact_products import F32, F64, KD_B, KD_DIM, KD_SHAPES, POOL, Probe, Tally, _scale_b, _sign, dev_, full, gpu, kd_select

NAN = float("nan")
POISON = 0xA5                                            # what byte outputs are pre-filled with
SLOPE = F32(0.01)                                        # voxconv.hip: VX_SLOPE
MULT = (4, 2, 1)                                         # equal terms per class of the dW cases ...
CLOUDS = ((0, 1, 2, 3), (1, 3), (2,))                    # ... = the clouds (of four) in which class s has its gradient
POOL_SHAPES = ((3, 15), (1, 19))                         # (B, E): 24 groups -- two live waves and two that return in the second workgroup; 27 -- a padding group
VDX_B, VDX_E = 4, 19                                     # 2048 rows of y1, 108 pool groups: two chunks of VX_DWG = 64, cloud 2 astride
VDX_OFFS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))  # the live groups' lattice offset per cloud: 8 + 4 + 4 + 4 = 20 live groups
VDW1_B, VDW1_E = 4, 15                                   # 864 rows of y1: three chunks of VX_W1CH = 256 and one of 96
KDW_B = 4                                                # 200 rows: a chunk of KD_CH = 128 and one of 72 whose last 16-row step has 8 rows


def vox_edges(E):
    E1 = (E - 5) // 2 + 1
    return E1, E1 - 2, (E1 - 2) // 2


def _fl32(x):
    return np.asarray(x, F64).astype(F32).astype(F64)


def _signed_a(p):
    """a of pair p with b's sign moved onto it: the other operand can then be |b| (a LeakyReLU / BN+ReLU identity passes it)"""
    return float(POOL.a[p]) * float(np.sign(POOL.b[p]))


# ---- conv2 + pool forward ---------------------------------------------------------------------------------------------------------
def pool_operands(B, E):
    """im2col form: A [B E2^3, 27 * 32] (k = tap * 32 + ci), B = wk [32, 864]; expect = the pre-pool tensor.  Also y1, w2 [32, 32, 27], the pooled
    output in the source's flatten order, the winner bytes, the share of strict maxima and the wins per member"""
    E1, E2, Ep = vox_edges(E)
    ids = POOL.pairs(1)
    y1 = np.zeros((B, E1, E1, E1, 32), F64)
    lat = 0
    for b in range(B):
        for z in range(b % 3, E1, 3):
            for y in range((b + 1) % 3, E1, 3):
                for x in range((b + 2) % 3, E1, 3):
                    ci = (7 * lat + 3) % 32
                    y1[b, z, y, x, ci] = float(POOL.a[ids[ci % ids.size]]) * 2.0 ** (((z + 2 * y + 3 * x) % 7) - 3)
                    lat += 1
    co, ci, tap = np.meshgrid(np.arange(32), np.arange(32), np.arange(27), indexing="ij")
    sg = [np.where((co >> i) & 1, -1, 1) for i in range(3)]
    ex = sg[0] * 4 * (tap // 9 - 1) + sg[1] * 2 * ((tap // 3) % 3 - 1) + sg[2] * (tap % 3 - 1) + (ci % 3) - 1
    w2 = np.abs(POOL.b[ids[ci % ids.size]].astype(F64)) * 2.0 ** ex
    A = np.zeros((B * E2 ** 3, 27 * 32), F64)
    for t in range(27):
        tz, ty, tx = t // 9, (t // 3) % 3, t % 3
        A[:, 32 * t:32 * t + 32] = y1[:, tz:tz + E2, ty:ty + E2, tx:tx + E2].reshape(-1, 32)
    Bm = w2.transpose(0, 2, 1).reshape(32, 27 * 32)
    kk = np.nonzero(A)[1]
    assert ((A != 0).sum(axis=1) == 1).all(), "every 3-wide window holds exactly one lattice point"
    pr = Probe(A, Bm, _fl32(A @ Bm.T), {int(p): 1 for p in set(ids[(kk % 32) % ids.size])})
    pr.taps, pr.cis = np.unique(kk // 32), np.unique(kk % 32)
    pre = pr.expect.reshape(B, Ep, 2, Ep, 2, Ep, 2, 32).transpose(0, 1, 3, 5, 2, 4, 6, 7).reshape(B * Ep ** 3, 8, 32)      # [group][member dz 4 + dy 2 + dx][c]
    assert (pre > 0).all()
    best = pre.max(axis=1)
    pr.win = pre.argmax(axis=1).astype(np.uint8)                                       # (the first maximum in member order)
    pr.strict = float(((pre == best[:, None, :]).sum(axis=1) == 1).mean())
    pr.wins = np.bincount(pr.win.reshape(-1), minlength=8)
    pr.out = np.ascontiguousarray(best.reshape(B, Ep ** 3, 32).transpose(0, 2, 1)).reshape(B, 32 * Ep ** 3)
    pr.y1, pr.w2 = y1.reshape(-1, 32).astype(F32), w2.astype(F32)
    return pr


# ---- conv2 backward: dX -------------------------------------------------------------------------------------------------------------
def vdx_operands(case):
    """A [B E1^3, 27 * 32] (k = tap * 32 + co): the dY a row of y1 meets through tap; B = wt [32 (ci), 864]; expect = the accumulator.  Live group
    number i has its gradient in channel (i + 20 case) % 32 at member (i + case) % 8"""
    B, E = VDX_B, VDX_E
    E1, E2, Ep = vox_edges(E)
    ids = POOL.pairs(1)
    pk = ids[np.arange(32) % ids.size]                                                 # the pair is a function of co: gout is seen through every tap
    gout = np.zeros((B, Ep, Ep, Ep, 32), F64)                                          # channel-last; the entry point takes [B][c Ep^3 + p]
    G_, c_ = np.meshgrid(np.arange(B * Ep ** 3), np.arange(32), indexing="ij")
    win = ((3 * G_ + 5 * c_ + case) % 8).astype(np.uint8)                              # decoys
    A = np.zeros((B, E1, E1, E1, 27 * 32), F64)
    live, cos, members = 0, [], []
    for b in range(B):
        oz, oy, ox = VDX_OFFS[b]
        for pz in range(oz, Ep, 2):
            for py in range(oy, Ep, 2):
                for px in range(ox, Ep, 2):
                    co, e = (live + 20 * case) % 32, (live + case) % 8
                    v = float(POOL.a[pk[co]]) * 2.0 ** ((live % 7) - 3) * (-1.0 if live % 3 == 0 else 1.0)
                    gout[b, pz, py, px, co] = v
                    win[(b * Ep + pz) * Ep * Ep + py * Ep + px, co] = e
                    qz, qy, qx = 2 * pz + (e >> 2), 2 * py + ((e >> 1) & 1), 2 * px + (e & 1)
                    for t in range(27):
                        A[b, qz + t // 9, qy + (t // 3) % 3, qx + t % 3, 32 * t + co] = v
                    cos.append(co), members.append(e)
                    live += 1
    A = A.reshape(B * E1 ** 3, 27 * 32)
    ci, k = np.meshgrid(np.arange(32), np.arange(27 * 32), indexing="ij")
    Bm = POOL.b[pk[k % 32]].astype(F64) * _scale_b(ci, k) * _sign(ci, k)
    pr = Probe(A, Bm, _fl32(A @ Bm.T), {int(p): 1 for p in set(pk[cos])})
    pr.live, pr.cos, pr.members, pr.taps = live, set(cos), set(members), np.unique(np.nonzero(A)[1] // 32)
    pr.w2 = np.ascontiguousarray(Bm.reshape(32, 27, 32).transpose(2, 0, 1)).astype(F32)                # [ci][tap][co] -> [co][ci][tap]
    pr.gout = np.ascontiguousarray(gout.reshape(B, Ep ** 3, 32).transpose(0, 2, 1)).reshape(B, 32 * Ep ** 3).astype(F32)
    pr.gp, pr.win = gout.reshape(B * Ep ** 3, 32).astype(F32), win
    row, c = np.meshgrid(np.arange(B * E1 ** 3), np.arange(32), indexing="ij")
    pr.y1 = ((0.5 + ((7 * row + c) % 11) / 8.0) * np.where((row + 3 * c) % 5 == 2, -1.0, 1.0)).astype(F32)
    pr.neg = pr.y1 < 0
    pr.dz = np.where(pr.neg, SLOPE * pr.expect, pr.expect)                              # float32 x float32: one rounding
    assert pr.dz.dtype == F32
    return pr


# ---- conv2 backward: dW ---------------------------------------------------------------------------------------------------------------
def vdw2_operands(which):
    """A = dY^T [32, NG * 8] (k = group * 8 + member), B [32 * 27 (ci * 27 + tap), NG * 8] = a1 at that member's position + tap; expect = dW2 in the
    source's order [co][ci][tap].  One pair per case"""
    B, E = VDX_B, VDX_E
    E1, E2, Ep = vox_edges(E)
    ep3, NG = Ep ** 3, B * Ep ** 3
    p = int(POOL.pairs(4)[which])
    pos, ci = np.meshgrid(np.arange(E1 ** 3), np.arange(32), indexing="ij")
    y1c = (abs(float(POOL.b[p])) * _scale_b(ci, pos)).reshape(E1, E1, E1, 32)
    co = np.arange(32)
    cls, grp, mem = co % 3, (5 * co + 2) % ep3, (3 * co + 1) % 8
    gv = _signed_a(p) * 2.0 ** ((co % 7) - 3) * _sign(co, 1)
    gp = np.zeros((NG, 32), F64)
    G_, c_ = np.meshgrid(np.arange(NG), co, indexing="ij")
    win = ((G_ + 3 * c_) % 8).astype(np.uint8)                                          # decoys: they select a zero
    A = np.zeros((32, NG * 8), F64)
    for c in co:
        for b in range(B):
            win[b * ep3 + grp[c], c] = mem[c]
        for b in CLOUDS[cls[c]]:
            gp[b * ep3 + grp[c], c] = gv[c]
            A[c, (b * ep3 + grp[c]) * 8 + mem[c]] = gv[c]
    P = np.zeros((ep3, 8, 27, 32), F64)
    for g in range(ep3):
        pz, py, px = g // (Ep * Ep), (g // Ep) % Ep, g % Ep
        for e in range(8):
            z, y, x = 2 * pz + (e >> 2), 2 * py + ((e >> 1) & 1), 2 * px + (e & 1)
            P[g, e] = y1c[z:z + 3, y:y + 3, x:x + 3].reshape(27, 32)
    Bm = np.tile(P.transpose(3, 2, 0, 1).reshape(32 * 27, 1, ep3 * 8), (1, B, 1)).reshape(32 * 27, NG * 8)
    pr = Probe(A, Bm, _fl32(A @ Bm.T), {p: 4})
    pr.gp, pr.win, pr.y1 = gp.astype(F32), win, np.tile(y1c.reshape(1, -1, 32), (B, 1, 1)).reshape(-1, 32).astype(F32)
    pr.db = (np.asarray(MULT, F64)[cls] * gv).astype(F32)
    pr.dw = pr.expect.reshape(32, 32, 27)
    pr.chunks = {int(c): sorted({(b * ep3 + grp[c]) // 64 for b in CLOUDS[cls[c]]}) for c in co}
    return pr


# ---- conv1 backward: dW ---------------------------------------------------------------------------------------------------------------
def vdw1_operands(which):
    """A = dz^T [32, B E1^3], B [125, B E1^3] = the input under tap of that row's patch; expect = dW1 [32, 125].  One pair per case"""
    B, E = VDW1_B, VDW1_E
    E1 = vox_edges(E)[0]
    e13 = E1 ** 3
    p = int(POOL.pairs(4)[which])
    i = np.arange(E ** 3)
    xc = (float(POOL.b[p]) * 2.0 ** (((5 * i) % 9) - 4) * np.where(i % 3 == 0, -1.0, 1.0)).reshape(E, E, E)
    co = np.arange(32)
    cls, row = co % 3, (41 * co + 7) % e13
    dv = float(POOL.a[p]) * 2.0 ** ((co % 7) - 3) * _sign(co, 1)
    dz = np.zeros((B * e13, 32), F64)
    for c in co:
        for b in CLOUDS[cls[c]]:
            dz[b * e13 + row[c], c] = dv[c]
    P = np.zeros((125, E1, E1, E1), F64)
    for t in range(125):
        tz, ty, tx = t // 25, (t // 5) % 5, t % 5
        P[t] = xc[tz:tz + 2 * E1:2, ty:ty + 2 * E1:2, tx:tx + 2 * E1:2]
    Bm = np.tile(P.reshape(125, 1, e13), (1, B, 1)).reshape(125, B * e13)
    pr = Probe(dz.T, Bm, _fl32(dz.T @ Bm.T), {p: 4})
    pr.dz, pr.x = dz.astype(F32), np.tile(xc.reshape(1, -1), (B, 1)).astype(F32)
    pr.chunks = sorted({int(b * e13 + row[c]) // 256 for c in co for b in CLOUDS[cls[c]]})
    return pr


# ---- kd level backward ------------------------------------------------------------------------------------------------------------------
def kd_rows_of(sel):
    """pre-pool row n of a cloud, s = sel[n], j = 3 n + s -> conv plane j / dim, source point j % dim (csrc/kdlevel.h)"""
    j = 3 * np.arange(KD_DIM)[None, :] + sel
    return j // KD_DIM, j % KD_DIM


def kd_decoys(B, F):
    """a pooled gradient that is non-zero everywhere under out = 0, with either parity in the winner byte: nothing of it may arrive"""
    r, f = np.meshgrid(np.arange(B * KD_DIM // 2), np.arange(F), indexing="ij")
    gout = 1.5 * 2.0 ** (((r + 2 * f) % 5) - 2) * np.where((r + f) % 3 == 0, -1.0, 1.0)
    return gout, np.zeros(gout.shape, F64), ((r + f) % 2).astype(np.uint8)


def kdx_operands(cin, F):
    """A [B dim (source rows), 3F] (k = 3 f + plane): the dy that a source point is fed; B = W^T [Cin, 3F]; expect = dX.  The live element of
    pooled row r is feature (7 r + 3) % F; its winner parity is the first of (r + b) % 2 and the other whose source no live row feeds yet.  Seen from
    the pair's second row the same element carries the other parity: that row's source expects a zero, or the term of another row"""
    B, dim = KD_B, KD_DIM
    sel = kd_select()
    k, p = kd_rows_of(sel)
    ids = POOL.pairs(1)
    pk = ids[np.arange(3 * F) % ids.size]
    c, kk = np.meshgrid(np.arange(cin), np.arange(3 * F), indexing="ij")
    Bm = np.abs(POOL.b[pk[kk]].astype(F64)) * _scale_b(c, kk)
    gout, out, win = kd_decoys(B, F)
    A = np.zeros((B * dim, 3 * F), F64)
    planes, feats, used = np.zeros((B, 3), np.int64), set(), set()
    for b in range(B):
        taken = set()
        for rl in range(dim // 2):
            r = b * (dim // 2) + rl
            for par in ((rl + b) % 2, 1 - (rl + b) % 2):
                n = 2 * rl + par
                if int(p[b, n]) not in taken:
                    break
            else:
                continue                                                               # (both sources are fed already: the pooled row stays dead)
            taken.add(int(p[b, n]))
            f = (7 * r + 3) % F
            q = 3 * f + int(k[b, n])
            v = _signed_a(pk[q]) * 2.0 ** ((r % 7) - 3) * float(_sign(r, 1))
            gout[r, f], out[r, f], win[r, f] = v, 1.25, par
            A[b * dim + int(p[b, n]), q] = v
            planes[b, k[b, n]] += 1
            feats.add(f % 16), used.add(int(pk[q]))
    pr = Probe(A, Bm, _fl32(A @ Bm.T), {q: 1 for q in used})
    pr.sel, pr.gout, pr.out, pr.win, pr.w = sel, gout.astype(F32), out.astype(F32), win, np.ascontiguousarray(Bm.T).astype(F32)
    pr.planes, pr.feats, pr.share = planes, feats, float((A != 0).any(axis=1).mean())
    return pr


def kdw_operands(cin, F):
    """A [3F, B dim (pre-pool rows)] = the dy of the rows of a channel's plane, B [Cin, B dim] = x at each row's source; expect = dW [3F, Cin].
    Class (q, s) has MULT[s] pooled rows, one in each cloud of CLOUDS[s], whose winner row lies in plane q; feature f has its gradient in class f % 3
    of every plane; the x rows of a class are identical, every other one is a decoy"""
    B, dim = KDW_B, KD_DIM
    M = B * dim
    sel = ((np.arange(B)[:, None] * 5 + np.arange(dim)[None, :] * 7) % 3).astype(np.int32)
    k, p = kd_rows_of(sel)
    pair = np.array([POOL.pairs(n)[(7 * s + 1) % POOL.pairs(n).size] for s, n in enumerate(MULT)])
    f_, c_ = np.arange(F), np.arange(cin)
    gv = np.array([_signed_a(pair[f % 3]) for f in f_]) * 2.0 ** ((f_ % 7) - 3) * _sign(f_, 1)
    ids = POOL.pairs(1)
    mm, cc = np.meshgrid(np.arange(M), c_, indexing="ij")
    X = np.abs(POOL.b[ids[(mm + cc) % ids.size]].astype(F64)) * _scale_b(cc, mm)        # decoys
    gout, out, win = kd_decoys(B, F)
    A = np.zeros((3 * F, M), F64)
    rows_used, src_used, live_rows = set(), set(), []
    for q in range(3):
        for s in range(3):
            xrow = abs(float(POOL.b[pair[s]])) * _scale_b(c_, 2 * (3 * q + s))
            for b in CLOUDS[s]:
                order = range(dim - 1, -1, -1) if b == 3 else range((7 * s + 3 * q) % dim, dim + (7 * s + 3 * q) % dim)
                for n in (t % dim for t in order):                                        # (cloud 3 from the top: the ragged last k step)
                    if k[b, n] == q and (b, n // 2) not in rows_used and (b, int(p[b, n])) not in src_used:
                        break
                else:
                    raise AssertionError("no free row of plane %d in cloud %d" % (q, b))
                rows_used.add((b, n // 2)), src_used.add((b, int(p[b, n])))
                live_rows.append(b * dim + n)
                X[b * dim + int(p[b, n])] = xrow
                r = (b * dim + n) // 2
                on = f_ % 3 == s
                gout[r, on], out[r, on], win[r, on] = gv[on], 1.25, n & 1
                A[3 * f_[on] + q, b * dim + n] = gv[on]
    src = (np.arange(B)[:, None] * dim + p).reshape(-1)
    pr = Probe(A, X[src].T, _fl32(A @ X[src]), {int(q): int(n) for q, n in zip(pair, MULT)})
    pr.sel, pr.gout, pr.out, pr.win, pr.x = sel, gout.astype(F32), out.astype(F32), win, X.astype(F32)
    pr.db = (np.asarray(MULT, F64)[np.repeat(f_, 3) % 3] * np.repeat(gv, 3)).astype(F32)                # dbias[3 f + q] = n g
    pr.live_rows = sorted(live_rows)
    return pr


# ---- the self-check -----------------------------------------------------------------------------------------------------------------------
def _all_probes():
    for B, E in POOL_SHAPES:
        yield "vox conv2 pool B %d E %d" % (B, E), pool_operands(B, E)
    for case in (0, 1):
        yield "vox conv2 dX, case %d" % case, vdx_operands(case)
    for which in (0, 2):
        yield "vox conv2 dW, pair %d" % which, vdw2_operands(which)
        yield "vox conv1 dW, pair %d" % which, vdw1_operands(which)
    for cin, f in KD_SHAPES:
        yield "kd dX %d <- 3 x %d" % (cin, f), kdx_operands(cin, f)
        yield "kd dW %d x 3 x %d" % (cin, f), kdw_operands(cin, f)


def test_every_loader_case():
    """every operand set through Probe.verify() (accepted pairs, no more equal terms than a pair admits, the expectation against an independent
    float64 product, values within 2^+-20), and the conditions the cases lean on"""
    assert POOL.pairs(4).size >= 3
    n = 0
    for name, pr in _all_probes():
        pr.verify()
        n += 1
    for B, E in POOL_SHAPES:
        pr = pool_operands(B, E)
        print("[loaders] pool B %d E %d: strict share %.3f, wins per member %s, %d ci" % (B, E, pr.strict, pr.wins.tolist(), pr.cis.size))
        assert pr.strict >= 0.9 and (pr.wins > 0).all()
        assert pr.taps.size == 27 and pr.cis.size >= 16 and (pr.cis < 16).any() and (pr.cis >= 16).any()
    cos, members, taps = set(), set(), set()
    for case in (0, 1):
        pr = vdx_operands(case)
        nz = (pr.expect != 0).any(axis=1)
        assert pr.live == 20 and nz.sum() == 540 and nz.mean() >= 0.2
        assert (pr.neg & (pr.expect != 0)).sum() >= 1000 and (~pr.neg & (pr.expect != 0)).sum() >= 1000, "both sides of the LeakyReLU' gate carry terms"
        assert (pr.dz[pr.neg & (pr.expect != 0)] != pr.expect[pr.neg & (pr.expect != 0)]).all()
        cos |= pr.cos
        members |= pr.members
        taps |= set(pr.taps.tolist())
    assert cos == set(range(32)) and members == set(range(8)) and taps == set(range(27))
    for which in (0, 2):
        pr = vdw2_operands(which)
        assert (pr.expect != 0).all() and pr.expect.size == 27648
        assert any(v == [0, 1] for c, v in pr.chunks.items() if c % 3 == 0) and {tuple(v) for c, v in pr.chunks.items() if c % 3 == 2} == {(0,), (1,)}, \
            "sums across the chunk boundary, and cloud 2 on either side of it"
        pr = vdw1_operands(which)
        assert (pr.expect != 0).all() and pr.chunks == [0, 1, 2, 3]
    for cin, f in KD_SHAPES:
        pr = kdx_operands(cin, f)
        print("[loaders] kd dX %d <- 3 x %d: %.2f of the source rows non-zero, live rows per (cloud, plane) %s" % (cin, f, pr.share, pr.planes.tolist()))
        assert pr.share >= 1 / 3 and (pr.planes >= 5).all() and pr.feats == set(range(16))
        pr = kdw_operands(cin, f)
        assert (pr.expect != 0).all() and (pr.db != 0).all()
        assert pr.live_rows[0] < 128 <= pr.live_rows[-1] and pr.live_rows[-1] >= 192, "rows in both chunks and in the ragged last k step"
    print("[loaders] %d case operand sets verified" % n)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
def u8(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(dev)


def run_prep(dev, w2):
    """papc_voxconv2_prep_f32: wk = W2[co][tap][ci], wt = W2[ci][tap][co], compared with the NumPy transposes bit for bit"""
    w, wk, wt = dev_(w2, dev), full((32, 27, 32), NAN, dev), full((32, 27, 32), NAN, dev)
    _lib.check(_lib.load().papc_voxconv2_prep_f32(w.data_ptr(), wk.data_ptr(), wt.data_ptr(), _lib.stream_ptr()), "papc_voxconv2_prep_f32")
    assert np.array_equal(wk.cpu().numpy().view(np.int32), np.ascontiguousarray(w2.transpose(0, 2, 1)).view(np.int32)) and \
        np.array_equal(wt.cpu().numpy().view(np.int32), np.ascontiguousarray(w2.transpose(1, 2, 0)).view(np.int32)), "wk / wt are not the transposes of w2"
    return wk, wt


@gpu
def test_voxconv2_prep(dev):
    """on a w2 whose 27 648 elements are all different, so that a misplaced one shows"""
    run_prep(dev, (1.0 + np.arange(32 * 32 * 27, dtype=F64).reshape(32, 32, 27) * 2.0 ** -15).astype(F32))


@gpu
@pytest.mark.parametrize("B,E", POOL_SHAPES)
def test_voxconv2_pool_forward(dev, B, E):
    """vox_conv2_pool_kernel (voxconv.hip:149): scale 1, shift 0, no bias -- the pooled value is the largest of eight exact single terms, the winner
    byte the first maximum in member order"""
    lib = _lib.load()
    Ep = vox_edges(E)[2]
    assert lib.papc_voxconv_ok(E) == 1
    pr = pool_operands(B, E)
    tally = Tally("vox conv2 + pool forward B %d E %d" % (B, E))
    wk, _ = run_prep(dev, pr.w2)
    y1, sc, sh = dev_(pr.y1, dev), torch.ones(32, device=dev), torch.zeros(32, device=dev)
    out, win = full((B, 32 * Ep ** 3), NAN, dev), full((B * Ep ** 3, 32), POISON, dev, torch.uint8)
    _lib.check(lib.papc_voxconv2_pool_fwd_f32(y1.data_ptr(), sc.data_ptr(), sh.data_ptr(), wk.data_ptr(), None, B, E, out.data_ptr(), win.data_ptr(),
                                              _lib.stream_ptr()), "papc_voxconv2_pool_fwd_f32")
    tally.add(out, pr.out, "out")
    tally.done()
    assert np.array_equal(win.cpu().numpy(), pr.win), "the winner bytes differ"


@gpu
@pytest.mark.parametrize("case", [0, 1])
def test_voxconv2_bwd_dx(dev, case):
    """vox_gp_kernel and vox_conv2_dx_kernel (voxconv.hip:231): mean 0, invstd 1, scale 1, shift 0.  gp is the channel-last copy of gout; dz the
    accumulator where y1 > 0 and fl32(0.01 acc) where y1 < 0; red_partial is written and not compared (sums: no exact image)"""
    lib = _lib.load()
    B, E = VDX_B, VDX_E
    E1, _, Ep = vox_edges(E)
    pr = vdx_operands(case)
    tally = Tally("vox conv2 dX, case %d" % case)
    _, wt = run_prep(dev, pr.w2)
    gout, win, y1 = dev_(pr.gout, dev), u8(pr.win, dev), dev_(pr.y1, dev)
    zero, one = torch.zeros(32, device=dev), torch.ones(32, device=dev)
    gp, dz = full((B * Ep ** 3, 32), NAN, dev), full((B * E1 ** 3, 32), NAN, dev)
    red = torch.empty(lib.papc_voxconv_parts(B, E), 2, 32, device=dev)
    _lib.check(lib.papc_voxconv2_bwd_dx_f32(gout.data_ptr(), win.data_ptr(), wt.data_ptr(), y1.data_ptr(), zero.data_ptr(), one.data_ptr(), one.data_ptr(),
                                            zero.data_ptr(), B, E, gp.data_ptr(), dz.data_ptr(), red.data_ptr(), _lib.stream_ptr()), "papc_voxconv2_bwd_dx_f32")
    tally.add(gp, pr.gp, "gp")
    tally.add(dz, pr.dz, "dz")
    tally.done()


@gpu
@pytest.mark.parametrize("which", [0, 2])
def test_voxconv2_bwd_dw(dev, which):
    """vox_conv2_dw_kernel (voxconv.hip:289), its chunk fold and vox_db2_kernel: scale 1, shift 0 on y1 > 0; sums of 4, 2, 1 equal terms"""
    lib = _lib.load()
    B, E = VDX_B, VDX_E
    pr = vdw2_operands(which)
    tally = Tally("vox conv2 dW, pair %d" % which)
    gp, win, y1 = dev_(pr.gp, dev), u8(pr.win, dev), dev_(pr.y1, dev)
    sc, sh = torch.ones(32, device=dev), torch.zeros(32, device=dev)
    nb = lib.papc_voxconv2_bwd_dw_workspace(B, E)
    assert nb == 2 * 27648 * 4
    ws, dw, db = full((nb // 4,), NAN, dev), full((32, 32, 27), NAN, dev), full((32,), NAN, dev)
    _lib.check(lib.papc_voxconv2_bwd_dw_f32(gp.data_ptr(), win.data_ptr(), y1.data_ptr(), sc.data_ptr(), sh.data_ptr(), B, E, dw.data_ptr(), db.data_ptr(), 0,
                                            ws.data_ptr(), nb, _lib.stream_ptr()), "papc_voxconv2_bwd_dw_f32")
    tally.add(dw, pr.dw, "dW2")
    tally.add(db, pr.db, "db2")
    tally.done()


@gpu
@pytest.mark.parametrize("which", [0, 2])
def test_voxconv1_bwd_dw(dev, which):
    """vox_conv1_dw_kernel (voxconv.hip:332) and its chunk fold: y1 = 0, mean 0, invstd 1, scale 1, c1 = c2 = 0, so dy1 = dz; db1 is the exact 0"""
    lib = _lib.load()
    B, E = VDW1_B, VDW1_E
    pr = vdw1_operands(which)
    tally = Tally("vox conv1 dW, pair %d" % which)
    dz, x, y1 = dev_(pr.dz, dev), dev_(pr.x, dev), torch.zeros(pr.dz.shape, device=dev)
    zero, one = torch.zeros(32, device=dev), torch.ones(32, device=dev)
    nb = lib.papc_voxconv1_bwd_dw_workspace(B, E)
    assert nb == 4 * 32 * 125 * 4
    ws, dw, db = full((nb // 4,), NAN, dev), full((32, 125), NAN, dev), full((32,), NAN, dev)
    _lib.check(lib.papc_voxconv1_bwd_dw_f32(dz.data_ptr(), y1.data_ptr(), zero.data_ptr(), one.data_ptr(), one.data_ptr(), zero.data_ptr(), zero.data_ptr(),
                                            x.data_ptr(), B, E, dw.data_ptr(), db.data_ptr(), 0, ws.data_ptr(), nb, _lib.stream_ptr()), "papc_voxconv1_bwd_dw_f32")
    tally.add(dw, pr.expect, "dW1")
    tally.add(db, np.zeros(32, F32), "db1")
    tally.done()


def run_kd_bwd(dev, pr, B, cin, F, x, w, want_dx):
    lib = _lib.load()
    dim = KD_DIM
    assert lib.papc_kdconv_ok(dim, cin, F) == 1
    gout, out, win, sel = dev_(pr.gout, dev), dev_(pr.out, dev), u8(pr.win, dev), dev_(pr.sel, dev)
    nb = lib.papc_kdconv_bwd_workspace(B, dim, cin, F)
    ws = full((nb // 4,), NAN, dev)
    dx = full((B * dim, cin), NAN, dev) if want_dx else None
    dw, db = full((3 * F, cin), NAN, dev), full((3 * F,), NAN, dev)
    _lib.check(lib.papc_kdconv_bwd_f32(gout.data_ptr(), out.data_ptr(), win.data_ptr(), x.data_ptr(), cin, sel.data_ptr(), dim, w.data_ptr(), B, dim, cin, F,
                                       _lib.ptr(dx), cin, dw.data_ptr(), db.data_ptr(), 0, ws.data_ptr(), nb, _lib.stream_ptr()), "papc_kdconv_bwd_f32")
    torch.cuda.synchronize()
    return dx, dw, db


@gpu
@pytest.mark.parametrize("cin,f", KD_SHAPES)
def test_kdconv_bwd_dx(dev, cin, f):
    """kd_dx_kernel / kd_dx_acc (kdlevel.h:135; Cin >= 32: papc_kdconv_bwd_f32 launches it whenever dx is given): one term per fed source row,
    exact zeros elsewhere; x holds decoys (dX does not read it)"""
    pr = kdx_operands(cin, f)
    tally = Tally("kd conv dX %d <- 3 x %d" % (cin, f))
    x = dev_(np.abs(pr.expect).astype(F32) + F32(1), dev)
    dx, _, _ = run_kd_bwd(dev, pr, KD_B, cin, f, x, dev_(pr.w, dev), True)
    tally.add(dx, pr.expect, "dX")
    tally.done()


@gpu
@pytest.mark.parametrize("cin,f", KD_SHAPES)
def test_kdconv_bwd_dw(dev, cin, f):
    """kd_dw_kernel / kd_dw_acc<1> (kdlevel.h:207; Cin >= 32) folded by papc_reduce_partials2_f32: dW as sums of 4, 2, 1 equal terms over both
    chunks, dbias = n g; w holds decoys (dW does not read it)"""
    pr = kdw_operands(cin, f)
    tally = Tally("kd conv dW %d x 3 x %d" % (cin, f))
    w = dev_(np.abs(pr.expect).astype(F32) + F32(1), dev)
    _, dw, db = run_kd_bwd(dev, pr, KDW_B, cin, f, dev_(pr.x, dev), w, False)
    tally.add(dw, pr.expect, "dW")
    tally.add(db, pr.db, "dbias")
    tally.done()
