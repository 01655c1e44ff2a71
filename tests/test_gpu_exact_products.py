"""Every GEMM flavour of the set-abstraction path held to the EXACT fp32 product, bit for bit, on three-plane probes.

Every matrix product on the hot path runs fp32 operands as three bf16 planes and six v_mfma_f32_32x32x16_bf16 products per block
(papc_amd/csrc/bf16x3.h).  The scheme is written once; the product loop is written 18 times, and each kernel stages its planes itself.  A
dropped product, a low-order product issued twice, planes 1 and 2 swapped on one staging path or a plane zeroed in a k-tail guard changes a
result by 2^-16 .. 2^-18 of a product: the size of honest fp32 rounding, far under the 1e-5 / 2e-4 bars of tests/util.py::assert_close.  No
tolerance separates "five of six products" from rounding.  Operand bits do.

The probe.  a = 1 + 2^-9 + 2^-18 splits into the planes (1, 2^-9, 2^-18), b = 1 + 2^-10 + 2^-20 into (1, 2^-10, 2^-20).  Their six kept
products are six distinct powers of two, the three dropped ones lie under half an ulp, so the six-product value IS fl32(a b), with one bit per
product.  A dot product with ONE non-zero term, or n <= 8 EQUAL terms, must therefore come out as n fl32(a b), bit for bit, from every flavour:
bf16x3, the true-fp32 MFMA flavours (PAPC_GEMM_F32 / PAPC_DW_F32) and the scalar loaders' paths.  The reference is the float64 product rounded to
fp32; the comparison is on the int32 view (-0 counted as +0); there is no tolerance.

test_probe_pool_and_every_case (NumPy, runs everywhere) screens a pool of candidate pairs -- three hand-made ones (the pair above, its signed
twin, (1.5 + 2^-9 + 2^-18, 1.25 + 2^-10 + 2^-20)), the square (b, b), a random family with a 7-bit leading plane and one with a 2-bit leading
plane -- and keeps a pair only if (i) both operands have three non-zero planes, (ii) the six products in
bf16x3.h's order give fl32 of the float64 product, (iii) each single drop, each single duplicate and the plane-1/2 swap of either operand
changes the bits, (iv) EVERY partial sum that n copies of the six products can form, in any order and any association, is a float32
(n sum|p_t| <= 2^24 times the products' lowest bit), and the fp32 fma chain reaches n fl32(a b) too.  (iv) is stricter than a fixed summation
order needs, on purpose: nothing then depends on how an MFMA adds inside.  It rejects most of the wide family (leading plane
1 + i 2^-7): accepted 35 of 132, of which 10 / 5 / 3 admit 2 / 4 / 8 equal terms.  A case that draws from a rejected pair, or sums more
terms than its pair admits, fails the self-check; every case's expectation is re-derived there by an independent float64 matrix product.

Layouts.  Forward / dX / planes: the sparse side has one non-zero per row at k(m) = (5 m + 3) mod K (7 m where 5 | K; every k including the ragged tail, every
row and column of a 32 x 32 fragment, two and more k blocks); the dense side holds probe values with a per-(n, k) power-of-two scale and sign,
so a wrong pairing of k shows in the exponent and a wrong plane in the low bits.  dW: dY is non-zero in one row per group (5 - 8 rows, in both
row chunks), in classes of 4, 2, 1 identical rows, so every dW element is a sum of 4, 2 or 1 equal terms folded across chunks; X is dense
(decoys in every other row).  The operand transforms are identities: A_BNRELU with scale 1 / shift 0 on A >= 0, A_GROUP with new_xyz = 0,
papc_bwd_dy with mean = 0, invstd = scale = shift = 1, y = 0, c1 = c2 = 0, wrow = 1.  Bias is zero.  Values stay within 2^+-20.

The 18 product loops and the case that reaches each.  How it is known: the dispatch condition cited (the profiler's PAPC_K_* families do
not tell kernels of one family apart, so launch counts are not used).
  mlp_gemm.hip:309   (TL: operands swapped)  test_tiled_dx, PAPC_GEMM_TL=1, f32 = 0: launch_gemm:925 (vec, dense dx, Cin % 4 == 0; with next_red Cin <= 64)
  mlp_gemm.hip:310   test_tiled_forward / _grouped / test_tiled_dx (tl = 0), f32 = 0.  M = 200 % 32 != 0 resp. PAPC_STREAM=0 decline stream_gemm_try
                     (mlp_stream.hip:987-988); BF3 = !PAPC_GEMM_F32 (GEMM_LAUNCH).  Instantiations: <4,1,1,1>, <2,2,2,1>, <2,4,2,1>, <2,2,2,2>, KB 1 / 2,
                     VEC and scalar, A_PLAIN / A_BNRELU / A_GROUP / A_DY_DENSE / A_DY_MAX, EPI_STORE / EPI_STORE_RED.  f32 = 1: the 32x32x2 f32 loop at :328-336
  mlp_stream.hip:392 (A_XYZ operand)  NOT reached: only a_mode == PAPC_A_XYZ dispatches it (mlp_gemm.hip:1064-1069); the operand is
                     relu(wf . xyz + t) recomputed per row -- an fma chain of the inputs, no image of one input value, and its k cannot vary with the row
  mlp_stream.hip:516 test_streaming_forward (a device-side row count has no other kernel: mlp_gemm.hip:918-921), test_compacted_dx (likewise), and
                     test_streaming_dx where stream_pick has the flavour (DENSE / MAX with next_red; DENSE alone for Cout 64 / 128: :963-972); elsewhere
                     that test runs the tiled kernel against the same expectation
  ... its PAPC_STREAM_ASM flavour   the asm = 1 cases of the three tests (ASM selects the hidden operand ring, stream_go:904; the MFMA loop is :516 either
                     way); asm = 0 has no ragged-k / ragged-n flavour (:918): 196 -> 256 forward is then refused, which the test asserts
  mlp_dw.hip:459     (dw_ws_kernel)  test_dw, PAPC_DW_ROWS = PAPC_DW_ROWSX = 0 or M = 100 or a plain input, both widths >= 64, Cin % 4 == 0 (launch_dw_v:1364);
                     <1,1,64> with PAPC_DW_RS64, <1,1>, <2,1>, <1,2>, <2,2>
  mlp_dw.hip:725     (dw_rows_kernel)  test_dw, M = 112, A_BNRELU, 64 -> 64, 64 -> 128, 128 -> 64, default knobs (:1358)
  mlp_dw.hip:938/969 (dw_rowsx_kernel: last blocks / weave)  test_dw, M = 112, A_BNRELU, 128 -> 128 (NW 4), 128 -> 256 (NW 8), the ragged pairs
                     128 -> 196, 196 -> 256, 96 -> 128, 64 -> 96 (:1340-1354).  Chunk 0 has four 16-row blocks: three in weave (:969), the last in mma (:938)
  mlp_dw.hip:1179-81 (dw_rows_max_kernel)  test_dw_max_without_stored_output: T on :1179 / :1180, the Gram matrix on :1181 ("gram": the pair (b, b))
  (dw_kernel, the staged true-fp32 kernel: test_dw under PAPC_DW_F32=1, and 13 -> 21, 32 -> 32 always)
  smallm.hip:489     (k16 ring)  test_planes, PAPC_PG_PIPE=1 (papc_pg_gemm_f32:885), NB 1 and 2, and pg_gemm_group_kernel<.., true>
  smallm.hip:609     (k32 stage loop)  test_planes, PAPC_PG_PIPE=0, and PAPC_PG_NS=3 under either value
  cloud_concat_k.hip:113   test_cloud_concat_k_forward (tier 2)
  kdlevel.h:50       (kd_step)  test_kdconv_forward (tier 2), through kd_fwd_acc
  kdlevel.h:263      (kd_dw_acc, which splits its own operands)  test_gpu_exact_loaders.py::test_kdconv_bwd_dw, see below
  voxconv.hip:58     (vox_step, the one product of all five voxconv kernels)  test_voxconv1_forward (tier 2), through vox_conv1_fwd_kernel's loader
  pfn.hip:404        test_pfn_apply (tier 2): k = 2, 3 as single terms, k = 0 + 7 and 1 + 8 as two equal terms; columns 4 - 6 (xyz - mean) cannot carry
                     an exact non-zero value
The six loaders that reach kd_step / vox_step / mfma_bf16x3 through a k loop and an on-load operand selection of their own -- each a separately
compiled kernel -- have their cases in the sibling file tests/test_gpu_exact_loaders.py (its docstring has the operand layouts):
  voxconv.hip:149    (vox_conv2_pool_kernel)  test_voxconv2_pool_forward: the one kernel of papc_voxconv2_pool_fwd_f32; (B, E) = (3, 15), (1, 19)
  voxconv.hip:231    (vox_conv2_dx_kernel, with vox_gp_kernel)  test_voxconv2_bwd_dx: the two launches of papc_voxconv2_bwd_dx_f32; E = 19, B = 4
  voxconv.hip:289    (vox_conv2_dw_kernel, its fold, vox_db2_kernel)  test_voxconv2_bwd_dw: papc_voxconv2_bwd_dw_f32; two chunks of VX_DWG = 64 groups
  voxconv.hip:332    (vox_conv1_dw_kernel and its fold)  test_voxconv1_bwd_dw: papc_voxconv1_bwd_dw_f32; three chunks of VX_W1CH = 256 rows and one of 96
  kdlevel.h:135      (kd_dx_kernel / kd_dx_acc on kd_step)  test_kdconv_bwd_dx: papc_kdconv_bwd_f32 with dx given, Cin >= 32 (kdconv.hip:184-188)
  kdlevel.h:207      (kd_dw_kernel / kd_dw_acc<1>, papc_reduce_partials2_f32)  test_kdconv_bwd_dw: papc_kdconv_bwd_f32, Cin >= 32 (kdconv.hip:197-202)
  (papc_voxconv2_prep_f32, which every conv2 case reads its weights through: test_voxconv2_prep and an assertion in each case)
What stays out: kdbn (kdbn.hip) always normalises its accumulator -- no exact image; the Cin = 3 kernels (kd_fwd3 / kd_dx3 / kd_dw3) are fmaf chains on
the vector unit, not MFMA loops.

Also pinned here: papc_pg_prep_rows_f32 writes planes_t for M % 128 != 0 inside its buffer (the planes_t cases have M = 32 and 64; before this
file the waves of a 128-row block behind M wrote zeros past a channel's k blocks and past the buffer).

Measured on the MI355X (every case, one run): 0 of N outputs differ in every family -- tiled forward 16 x 426 000 + 8 x 213 000 outputs,
row-streaming forward 13 cases (65 536 .. 262 144 each), tiled dX 24 cases (58 240 .. 878 080), streaming dX 32, compacted dX 3 x 32 768, dW 26
cases (1 092 .. 200 704), dW max 8 192 + 12 352, planes 12 cases (65 536 .. 278 528), cloud concat 3, kd conv 2, vox conv1 2, pfn apply 2.
The loaders (tests/test_gpu_exact_loaders.py, one run): 0 of N outputs differ in every family -- vox conv2 + pool forward 768 and 864 outputs (and every
winner byte), vox conv2 dX 2 x 68 992 (3 456 of gp, 65 536 of dz), vox conv2 dW 2 x 27 680 (27 648 + db2), vox conv1 dW 2 x 4 032 (4 000 + db1),
kd conv dX 3 200 and 9 600, kd conv dW 3 168 and 46 560 (dW + dbias); wk / wt equal the transposes in all five launches of the prep kernel.

What a broken loop does to this file was tried once, on a scratch build that is not in the tree: product 0 dropped at mlp_gemm.hip:304, planes
1 / 2 swapped in mlp_stream.hip's weight image, product 0 issued twice in smallm.hip's k16 ring, and pl[1] / pl[2] swapped in split8 (which
reached the sources rebuilt against that bf16x3.h: the dW rows / rowsx / max kernels and the planes prep kernels).  104 of the 145 tests then
in the file failed: every bf16x3 case of the tiled, row-streaming, compacted and planes kernels and of the split8-fed dW kernels.  The 41 that
passed: the true-fp32 flavours (f32 = 1), the dW cases that run dw_ws_kernel / dw_kernel under every knob, the refusals, and cloud_concat_k /
kdconv, whose objects were not rebuilt.

The same for the loaders, on a second scratch build loaded through PAPC_LIB: planes 1 / 2 of the A operand exchanged in vox_step, and product 0
(a3 b1) left out of a local copy of the product loop in kd_dw_acc.  10 of the 13 tests of tests/test_gpu_exact_loaders.py failed: every case of the four
voxconv loaders (pool forward 768 of 768 and 864 of 864 outputs, dX 17 280 of 65 536 -- every non-zero element of dz --, conv2 dW 27 648 of 27 648,
conv1 dW 4 000 of 4 000) and both kd dW cases (3 072 of 3 072, 46 080 of 46 080).  The 3 that passed: test_voxconv2_prep (a copy), and the two kd dX
cases, which run kd_step, left intact.  Within the failing cases gp, db2, db1 and dbias still agreed: none of them passes through an MFMA.
"""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib, smallm
from papc_amd._lib import BwdDy, BwdRed, GroupSrc
from tests.test_gpu_bf16x3 import bf16_to_f32, split3

gpu = pytest.mark.gpu          # (the self-check of the inputs is NumPy only and runs everywhere)

F32, F64 = np.float32, np.float64
PA, PB = (2, 1, 0, 1, 0, 0), (0, 1, 2, 0, 1, 0)          # csrc/bf16x3.h: BF16X3_PA / BF16X3_PB
A_PLAIN, A_BNRELU, A_GROUP = 0, 1, 2
DZ_DENSE, DZ_MAX = 0, 1
CAPACITY = 65536                                          # rows of the row-streaming kernels' capacity buffers


# ---- the probe pairs -------------------------------------------------------------------------------------------------------------
def _planes(x):
    """float32 [n] -> the three planes of the split, as float32 values"""
    s = split3(np.ascontiguousarray(x, F32).reshape(1, -1))
    return [bf16_to_f32(s[i])[0] for i in range(3)]


def six(a, b, drop=None, dup=None, swap_a=False, swap_b=False):
    """the six products of bf16x3.h in their documented order, accumulated in float32 (a product of two bf16 has 16 significand bits:
    the float32 multiplication is exact); ``drop`` / ``dup``: product t left out / issued twice; ``swap_*``: planes 1 and 2 of an operand
    exchanged"""
    A, B = _planes(a), _planes(b)
    if swap_a:
        A = [A[0], A[2], A[1]]
    if swap_b:
        B = [B[0], B[2], B[1]]
    acc = np.zeros(np.shape(a), F32)
    for t in range(6):
        if t == drop:
            continue
        p = A[PA[t]] * B[PB[t]]
        assert p.dtype == F32
        acc = acc + p
        if t == dup:
            acc = acc + p
    return acc


def _lowbit(v):
    """weight of the lowest set significand bit of every float64 in v (infinity for 0)"""
    m, e = np.frexp(np.abs(v))
    im = np.round(m * 2.0 ** 53).astype(np.int64)
    return np.where(v != 0, (im & -im).astype(F64) * 2.0 ** (e - 53.0), np.inf)


def _candidates():
    """three hand-made pairs, (b, b) of the first (the Gram product of the max layer's dW squares one operand), a random family with the leading
    plane 1 + i 2^-7 and the same family with two-bit leading planes (1 + i / 4), whose products leave room for sums of equal terms"""
    ha = [1 + 2.0 ** -9 + 2.0 ** -18, 1 - 2.0 ** -9 + 2.0 ** -18, 1.5 + 2.0 ** -9 + 2.0 ** -18, 1 + 2.0 ** -10 + 2.0 ** -20]
    hb = [1 + 2.0 ** -10 + 2.0 ** -20, -(1 + 2.0 ** -10 - 2.0 ** -20), 1.25 + 2.0 ** -10 + 2.0 ** -20, 1 + 2.0 ** -10 + 2.0 ** -20]
    rng = np.random.default_rng(20261021)

    def family(n, lead_bits):
        sgn = lambda: rng.choice([-1.0, 1.0], n)
        quarter = lambda: 1 + rng.integers(0, 4, n) * 0.25
        lead = lambda: 1 + rng.integers(0, 1 << lead_bits, n) * 2.0 ** -lead_bits
        return (lead() + sgn() * 2.0 ** -10 * quarter() + sgn() * 2.0 ** -20, lead() + sgn() * 2.0 ** -11 * quarter() + sgn() * 2.0 ** -21)

    a7, b7 = family(32, 7)
    a2, b2 = family(96, 2)
    a, b = np.concatenate([ha, a7, a2]), np.concatenate([hb, b7, b2])
    assert np.array_equal(a.astype(F32).astype(F64), a) and np.array_equal(b.astype(F32).astype(F64), b)      # every candidate IS a float32
    return a.astype(F32), b.astype(F32)


SQUARE = 3      # candidate (b, b) of the first pair


class Pool:
    """the candidates and what the self-check found: ``keep`` (i)-(iii) hold, ``nmax`` the largest n <= 8 of (iv)"""

    def __init__(self):
        self.a, self.b = _candidates()
        a, b = self.a, self.b
        A, B = _planes(a), _planes(b)
        self.three = np.all([p != 0 for p in A + B], axis=0)                                                    # (i)
        self.exact = (a.astype(F64) * b.astype(F64)).astype(F32)
        bits = self.exact.view(np.int32)
        self.six_ok = six(a, b).view(np.int32) == bits                                                          # (ii)
        broken = [six(a, b, drop=t) for t in range(6)] + [six(a, b, dup=t) for t in range(6)] + [six(a, b, swap_a=True), six(a, b, swap_b=True)]
        self.sensitive = np.all([x.view(np.int32) != bits for x in broken], axis=0)                             # (iii)
        # (iv), for every summation order and every association inside an MFMA: a sum of c_t <= n copies of product t is a multiple of the
        # products' smallest bit g and at most n S, S = sum |product|; n S <= 2^24 g makes every such partial sum a float32
        P = np.array([A[PA[t]].astype(F64) * B[PB[t]].astype(F64) for t in range(6)])
        g, S = _lowbit(P).min(axis=0), np.abs(P).sum(axis=0)
        nmax = np.clip(np.floor(2.0 ** 24 * g / S), 0, 8).astype(np.int64)
        # ... and the float32 fma chain of the true-fp32 MFMA flavours and the scalar paths, acc <- fl32(acc + a b): j fl32(a b) after j terms
        e64, p64 = self.exact.astype(F64), a.astype(F64) * b.astype(F64)
        for j in range(1, 9):
            ok = ((j - 1) * e64 + p64).astype(F32).astype(F64) == j * e64        # (24 + 48 significand bits three binades apart: exact in float64)
            nmax = np.where(ok, nmax, np.minimum(nmax, j - 1))
        self.nmax = nmax
        self.keep = self.three & self.six_ok & self.sensitive & (nmax >= 1)

    def pairs(self, n=1, exclude_square=True):
        ids = np.flatnonzero(self.keep & (self.nmax >= n))
        if exclude_square:
            ids = ids[ids != SQUARE]
        assert ids.size, "no probe pair admits sums of %d equal terms" % n
        return ids


POOL = Pool()


class Probe:
    """one case's operands in GEMM form, y[i, j] = sum_k A[i, k] B[j, k]: A sparse, B dense, ``expect`` from float64 NumPy; ``used`` = the
    candidates it draws from with the number of equal terms it sums of each"""

    def __init__(self, A, B, expect, used):
        self.A, self.B, self.expect, self.used = A.astype(F32), B.astype(F32), expect.astype(F32), used
        assert np.array_equal(self.A.astype(F64), A) and np.array_equal(self.B.astype(F64), B) and np.array_equal(self.expect.astype(F64), expect)

    def verify(self):
        """a rejected pair in a case is an error of the inputs; the expectation against an independent float64 product"""
        for p, n in self.used.items():
            assert POOL.keep[p] and n <= POOL.nmax[p], "the case draws %d equal terms from pair %d (keep %s, nmax %d)" % (n, p, POOL.keep[p], POOL.nmax[p])
        nz = (self.A != 0).sum(axis=1)
        assert nz.max() <= 8
        ref = self.A.astype(F64) @ self.B.astype(F64).T          # zeros and <= 8 equal 48-bit terms: exact in float64 in any order
        assert np.array_equal(ref.astype(F32), self.expect)
        big = max(np.abs(self.A).max(), np.abs(self.B).max(), np.abs(self.expect).max())
        small = min(np.abs(self.A[self.A != 0]).min(), np.abs(self.B[self.B != 0]).min(), np.abs(self.expect[self.expect != 0]).min())
        assert big <= 2.0 ** 20 and small >= 2.0 ** -20


def _scale_b(n, k):
    """per-(n, k) scale of the dense side: a power of two 2^-4 .. 2^4, so that a wrong pairing of k shows in the exponent"""
    return 2.0 ** (((3 * n + 5 * k) % 9) - 4)


def _sign(n, k):
    return np.where((n + 2 * k) % 3 == 0, -1.0, 1.0)


def single_term(M, N, K, sign_a=False, km=None):
    """A [M, K]: ONE non-zero per row, at k(m) = (s m + 3) mod K with s = 5 (7 where 5 divides K) -- every k where M >= K, every row and
    column of a 32 x 32 fragment, a k that varies with m; ``km`` overrides it (-1: an empty row).  B [N, K] dense.  The pair is a function
    of k.  Signs go on B (the weights: A >= 0 passes a BN+ReLU identity), with ``sign_a`` on A's rows as well"""
    ids = POOL.pairs(1)
    pk = ids[np.arange(K) % ids.size]
    m = np.arange(M)
    if km is None:
        step = 5 if K % 5 else 7
        assert np.gcd(step, K) == 1
        km = (step * m + 3) % K
        assert M < K or np.unique(km).size == K
    live = km >= 0
    kc = np.where(live, km, 0)
    A = np.zeros((M, K), F64)
    A[m[live], kc[live]] = (POOL.a[pk[kc]].astype(F64) * 2.0 ** ((m % 7) - 3) * (_sign(m, 1) if sign_a else 1.0))[live]
    n_, k_ = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    B = POOL.b[pk].astype(F64)[None, :] * _scale_b(n_, k_) * _sign(n_, k_)
    expect = (A[m, kc][:, None] * B[:, kc].T).astype(F32).astype(F64)      # fl32 of the exact float64 term
    return Probe(A, B, expect, {int(p): 1 for p in set(pk[kc[live]])})


def _mults(G):
    """multiplicities 4, 2, 1, 1, ... adding up to G: the numbers of equal terms of a dW case's row classes"""
    out, left = [], G
    for n in (4, 2):
        if left >= n + 1 or left == n:
            out.append(n)
            left -= n
    return out + [1] * left


def dw_operands(M, Cin, Cout, K):
    """dW[co, ci] = sum_m dY[m, co] X[m, ci] with dY non-zero in ONE row per group of K rows (M / K <= 8 rows in all, spread over the row
    chunks).  The rows form classes of 4, 2, 1, ... IDENTICAL rows (of dY and of X): channel co has its non-zeros in the rows of class
    co mod S, so dW[co, ci] is a sum of 4, 2 or 1 equal terms.  Every other row of X holds decoys.  X >= 0 (a BN+ReLU identity passes it);
    signs on dY.  Also the form the max-pooled flavours read: gout / argmax [M / K, Cout] with argmax the row offset inside the group.
    In GEMM form: A = dY^T [Cout, M] sparse, B = X^T [Cin, M] dense"""
    G = M // K
    assert G * K == M and 2 <= G <= 8
    mult = _mults(G)
    S = len(mult)
    cls = np.repeat(np.arange(S), mult)[(3 * np.arange(G)) % G] if np.gcd(3, G) == 1 else np.repeat(np.arange(S), mult)[::-1]
    assert sorted(np.bincount(cls, minlength=S).tolist()) == sorted(mult)
    rows = np.arange(G) * K + (3 * np.arange(G) + 1) % K
    pair = np.array([POOL.pairs(n)[(7 * s + 1) % POOL.pairs(n).size] for s, n in enumerate(mult)])
    co, ci = np.arange(Cout), np.arange(Cin)
    dyv = POOL.a[pair[co % S]].astype(F64) * 2.0 ** ((co % 7) - 3) * _sign(co, 1) * np.sign(POOL.b[pair[co % S]].astype(F64))
    ids = POOL.pairs(1)
    mm, cc = np.meshgrid(np.arange(M), ci, indexing="ij")
    X = np.abs(POOL.b[ids[(mm + cc) % ids.size]].astype(F64)) * _scale_b(cc, mm)                # decoys
    dY = np.zeros((M, Cout), F64)
    gout, argmax = np.zeros((G, Cout), F64), ((7 * np.arange(G)[:, None] + co[None, :]) % K).astype(np.int32)
    for g in range(G):
        s = cls[g]
        X[rows[g]] = np.abs(POOL.b[pair[s]].astype(F64)) * _scale_b(ci, 2 * s)
        on = co % S == s
        dY[rows[g], on] = dyv[on]
        gout[g, on] = dyv[on]
        argmax[g, on] = rows[g] - g * K
    first = np.array([rows[np.flatnonzero(cls == s)[0]] for s in range(S)])
    term = (dyv[:, None] * X[first[co % S]]).astype(F32).astype(F64)
    pr = Probe(dY.T, X.T, np.asarray(mult, F64)[co % S][:, None] * term, {int(p): int(n) for p, n in zip(pair, mult)})
    pr.dY, pr.X, pr.gout, pr.argmax, pr.rows = dY.astype(F32), X.astype(F32), gout.astype(F32), argmax, rows
    return pr


def gram_operands(M, K, Cin, Cout):
    """the max layer's dW without stored output forms T = P'^T A and the Gram matrix A^T A in one pass: X is zero but for ONE row r0, whose
    channels hold the value b of the first pair at per-channel scales, so G[i, j] = fl32(b b) 2^(e_i + e_j) is a single term -- candidate
    (b, b) -- and T[co, ci] = psel[g0, co] X[r0, ci] is one of the first pair"""
    r0 = 5 * K + 7
    g0 = r0 // K
    ci, co = np.arange(Cin), np.arange(Cout)
    X = np.zeros((M, Cin), F64)
    X[r0] = POOL.b[0].astype(F64) * 2.0 ** ((ci % 9) - 4)
    psel, argmax = np.zeros((M // K, Cout), F64), ((co[None, :] + np.arange(M // K)[:, None]) % K).astype(np.int32)
    psel[g0] = POOL.a[0].astype(F64) * 2.0 ** ((co % 7) - 3) * _sign(co, 1)
    argmax[g0] = r0 - g0 * K
    P = np.zeros((M, Cout), F64)
    P[r0] = psel[g0]
    t = Probe(P.T, X.T, (psel[g0][:, None] * X[r0][None, :]).astype(F32).astype(F64), {0: 1})
    gx = np.zeros((Cin, M), F64)
    gx[:, r0] = X[r0]
    g = Probe(gx, X.T, (X[r0][:, None] * X[r0][None, :]).astype(F32).astype(F64), {SQUARE: 1})
    return t, g, X.astype(F32), psel.astype(F32), argmax, X[r0].astype(F32)


def max_rows(M, Cout, K):
    """k(m) of a dX case under the max: one row per (group, channel), so a row whose channel an earlier row of its group holds stays empty"""
    km = (5 * np.arange(M) + 3) % Cout
    for g in range(M // K):
        seen = set()
        for m in range(g * K, (g + 1) * K):
            if km[m] in seen:
                km[m] = -1
            seen.add(km[m])
    return km


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
TILED_M = 200                                            # 128 + 72: a ragged last row tile
TILED_CIN, TILED_COUT = (13, 32, 64, 196), (21, 64, 128)
GROUP_D = (5, 16)
ROWS_DEV = 256
STREAM_SHAPES = ((64, 64), (128, 256), (96, 128), (196, 256))
DX_M, DX_K = 224, 32                                     # 128 + 96 rows, seven groups of 32
DX_TILED = ((21, 13), (64, 64), (128, 64), (256, 128), (196, 128), (256, 196))        # (Cout, Cin)
DX_STREAM = ((64, 64), (128, 64), (128, 128), (256, 64), (196, 128), (256, 196), (96, 64), (128, 96))
DW_CASES = (      # (Cin, Cout, a_mode, M, K): M = 100 has no whole 16-row blocks (the staged kernels); 112 = a 64-row chunk and a ragged one of 48
    (13, 21, A_PLAIN, 100, 20), (32, 32, A_BNRELU, 100, 20), (64, 64, A_BNRELU, 100, 20), (64, 64, A_PLAIN, 112, 16), (64, 64, A_BNRELU, 112, 16),
    (64, 128, A_BNRELU, 112, 16), (128, 64, A_BNRELU, 112, 16), (128, 128, A_BNRELU, 112, 16), (128, 256, A_BNRELU, 112, 16), (128, 196, A_BNRELU, 112, 16),
    (196, 256, A_BNRELU, 112, 16), (96, 128, A_BNRELU, 112, 16), (64, 96, A_BNRELU, 112, 16))
PG_R1, PG_R2, PG_K = 128, (64, 136), (32, 40)
CCK_B, CCK_N, CCK_CG = 2, 100, 64                        # two clouds of 100 points: the second 128-row tile is ragged and the first straddles the clouds
CCK_SHAPES = ((64, 64), (128, 128), (256, 192))          # (Cp, Cout): 64-column tiles, 128-column tiles, three 64-column blocks
KD_B, KD_DIM = 2, 50                                     # 100 pre-pool rows: three 32-row tiles and a ragged one
KD_SHAPES = ((32, 32), (96, 160))                        # (Cin, F)


VOX_B, VOX_E = 2, 15                                     # E1 = 6: 432 rows of y1, three 128-row workgroups and a ragged one


def vox_operands(which):
    """conv1 of the VoxNet backbone (5^3 taps, stride 2) as a single-term product: the non-zero voxels of a cloud lie on a lattice of period 6 per
    axis (offsets per axis and cloud), so the five-wide window of an output position holds at most one of them per axis -- y1[row, co] is one
    term at the tap that voxel has in the row's window, or an exact zero.  A voxel meets several taps, so ONE pair serves the whole case.
    Returns the grid x [B, E^3], and the probe in im2col form: A [B E1^3, 125], B = w1 [32, 125]"""
    B, E = VOX_B, VOX_E
    E1 = (E - 5) // 2 + 1
    pid = POOL.pairs(1)[which]
    x = np.zeros((B, E, E, E), F64)
    for b in range(B):
        offs = [(2 * ax + b) % 6 for ax in range(3)]
        zs, ys, xs = (np.arange(o, E, 6) for o in offs)
        zz, yy, xx = np.meshgrid(zs, ys, xs, indexing="ij")
        x[b, zz, yy, xx] = POOL.a[pid].astype(F64) * 2.0 ** (((zz + 2 * yy + 3 * xx) % 7) - 3)
    co, tap = np.meshgrid(np.arange(32), np.arange(125), indexing="ij")
    w1 = POOL.b[pid].astype(F64) * _scale_b(co, tap) * _sign(co, tap)
    A = np.zeros((B * E1 ** 3, 125), F64)
    for b in range(B):
        for oz in range(E1):
            for oy in range(E1):
                for ox in range(E1):
                    patch = x[b, 2 * oz:2 * oz + 5, 2 * oy:2 * oy + 5, 2 * ox:2 * ox + 5]
                    A[((b * E1 + oz) * E1 + oy) * E1 + ox] = patch.reshape(125)
    assert (A != 0).sum(axis=1).max() == 1 and (A != 0).any(axis=1).mean() > 0.2 and np.unique(np.nonzero(A)[1]).size >= 8
    return x.reshape(B, E ** 3), Probe(A, w1, (A @ w1.T).astype(F32).astype(F64), {int(pid): 1})


PFN_P, PFN_T = 70, 40                                    # 70 pillars over workgroups of four waves; 40 points: a full and a ragged 32-row tile


def pfn_operands(C):
    """PillarFeatureNet's decorated rows [x, y, z, r, xyz - mean, x - cx, y - cy] as a probe: a pillar at grid cell (0, 0) with offsets 0 (its
    centre is the origin) holds ONE point with ONE non-zero column j = p mod 4.  Then xyz - mean is an exact zero, column 7 repeats x and column
    8 repeats y, so with w[:, 7] = w[:, 0] and w[:, 8] = w[:, 1] an x or y pillar is a sum of TWO equal terms (k = 0 and 7, 1 and 8) and a z or r
    pillar a single term (k = 2, 3).  Reflectance does not enter the mean: an r pillar may have up to T real rows, the non-zero one last, which
    reaches the second row tile.  Everything positive: BN (scale 1, shift 0), ReLU and the max over the rows pass the product through"""
    P, T = PFN_P, PFN_T
    two, one = POOL.pairs(2), POOL.pairs(1)
    pair_k = [int(two[0]), int(two[1 % two.size]), int(one[3 % one.size]), int(one[7 % one.size])]
    feat, nv, A = np.zeros((P, T, 4), F64), np.ones(P, np.int32), np.zeros((P, 9), F64)
    for q in range(P):
        j = q % 4
        v = float(POOL.a[pair_k[j]]) * 2.0 ** ((q % 7) - 3)
        if j == 3:
            nv[q] = T if q % 8 == 3 else 1 + (5 * q) % T
        feat[q, nv[q] - 1, j] = v
        A[q, j] = v
        if j < 2:
            A[q, 7 + j] = v
    c = np.arange(C)
    w = np.zeros((C, 9), F64)
    for k in range(9):
        src = k - 7 if k >= 7 else k
        w[:, k] = np.abs(float(POOL.b[pair_k[src] if src < 4 else one[0]])) * _scale_b(c, src)
    used = {}
    for k, n in zip(pair_k, (2, 2, 1, 1)):
        used[k] = max(used.get(k, 0), n)
    return feat.astype(F32), nv, Probe(A, w, (A @ w.T).astype(F32).astype(F64), used)


def positive(pr):
    """the same probe with the signs taken off the dense side: every product is positive (a ReLU and a max pass it)"""
    return Probe(pr.A.astype(F64), np.abs(pr.B).astype(F64), np.abs(pr.expect).astype(F64), pr.used)


def kd_rows(sel):
    """kdnet.py:21-30 as csrc/kdlevel.h states it: pre-pool row n of a cloud, s = sel[n], j = 3 n + s -> conv plane k = j / dim, source point p = j % dim"""
    j = 3 * np.arange(KD_DIM)[None, :] + sel
    return j // KD_DIM, j % KD_DIM


def kd_select():
    return ((np.arange(KD_B)[:, None] * 5 + np.arange(KD_DIM)[None, :] * 7) % 3).astype(np.int32)


def _all_probes():
    for cin in TILED_CIN + tuple(d + 3 for d in GROUP_D):
        for cout in TILED_COUT:
            yield "forward %d -> %d" % (cin, cout), single_term(TILED_M, cout, cin)
    for cin, cout in STREAM_SHAPES:
        yield "rows %d -> %d" % (cin, cout), single_term(ROWS_DEV, cout, cin)
    for cout, cin in DX_TILED:
        yield "dX %d -> %d" % (cout, cin), single_term(DX_M, cin, cout, sign_a=True)
        yield "dX max %d -> %d" % (cout, cin), single_term(DX_M, cin, cout, sign_a=True, km=max_rows(DX_M, cout, DX_K))
    for cout, cin in DX_STREAM + ((256, 128),):
        yield "dX rows %d -> %d" % (cout, cin), single_term(ROWS_DEV, cin, cout, sign_a=True)
        yield "dX rows max %d -> %d" % (cout, cin), single_term(ROWS_DEV, cin, cout, sign_a=True, km=max_rows(ROWS_DEV, cout, DX_K))
    for cin, cout, _, M, K in DW_CASES:
        yield "dW %d -> %d" % (cin, cout), dw_operands(M, cin, cout, K)
    yield "dW max 64 -> 128", dw_operands(256, 64, 128, 32)
    t, g = gram_operands(256, 32, 64, 128)[:2]
    yield "dW max T", t
    yield "dW max Gram", g
    for r2 in PG_R2:
        for k in PG_K + (64,):
            yield "planes %d x %d x %d" % (PG_R1, r2, k), single_term(PG_R1, r2, k)
    for cp, cout in CCK_SHAPES:
        yield "cloud concat %d -> %d" % (cp, cout), single_term(CCK_B * CCK_N, cout, cp)
    for cin, f in KD_SHAPES:
        yield "kd conv %d -> 3 x %d" % (cin, f), positive(single_term(KD_B * KD_DIM, 3 * f, cin))
    for which in (0, 5):
        yield "vox conv1, pair %d" % which, vox_operands(which)[1]
    for C in (64, 40):
        yield "pfn apply, %d channels" % C, pfn_operands(C)[2]


def test_probe_pool_and_every_case():
    """(i)-(iv) of the module docstring on every candidate pair, in NumPy; then every case's operands: none draws from a rejected pair or sums more equal
    terms than its pair admits, its expectation equals an independent float64 product, and every value stays within 2^+-20"""
    p = POOL
    print("[pool] %d candidates: %d three-plane, %d with six products == fl32(exact), %d sensitive to every drop / duplicate / plane swap; accepted %d "
          "(rejected %d); sums of 2 / 4 / 8 equal terms exact in any order: %d / %d / %d pairs"
          % (p.a.size, p.three.sum(), (p.three & p.six_ok).sum(), (p.three & p.six_ok & p.sensitive).sum(), p.keep.sum(), (~p.keep).sum(),
             (p.keep & (p.nmax >= 2)).sum(), (p.keep & (p.nmax >= 4)).sum(), (p.keep & (p.nmax >= 8)).sum()))
    # the three hand-made pairs and the square are in: 8, 8 and 4 equal terms
    assert p.keep[:4].all() and p.nmax[0] == 8 and p.nmax[1] == 8 and 4 <= p.nmax[2] < 8, (p.keep[:4], p.nmax[:4])
    assert p.keep.sum() >= 16 and (p.keep & (p.nmax >= 2)).sum() >= 4 and (p.keep & (p.nmax >= 4)).sum() >= 2
    # what the self-check is for: it rejects most of the wide family (candidates 4 .. 35)
    assert not p.keep[4:36].all()
    # the emulation of a broken loop really differs: product 0 (a3 b1) of the first pair is its bit 2^-18
    assert float(six(p.a[:1], p.b[:1])[0]) - float(six(p.a[:1], p.b[:1], drop=0)[0]) == 2.0 ** -18
    n = 0
    for name, pr in _all_probes():
        pr.verify()
        n += 1
    print("[pool] %d case operand sets verified" % n)


# ---- GPU plumbing ----------------------------------------------------------------------------------------------------------------
KNOBS = ("PAPC_STREAM", "PAPC_STREAM_MINTILES", "PAPC_STREAM_ASM", "PAPC_STREAM_NW12", "PAPC_STREAM_MAXCAT", "PAPC_MAX_NOSTORE", "PAPC_GEMM_F32", "PAPC_GEMM_TL",
         "PAPC_GEMM_KB", "PAPC_GEMM_MINWG", "PAPC_GEMM_WAVES", "PAPC_DW_F32", "PAPC_DW_ROWS", "PAPC_DW_ROWSX", "PAPC_DW_RS64", "PAPC_PG_PIPE", "PAPC_PG_GROUP",
         "PAPC_PG_NB", "PAPC_PG_NS", "PAPC_PFN_MFMA")


@pytest.fixture
def knob():
    """knob(name, value) sets a knob of the library; every knob this file touches is put back afterwards"""
    lib = _lib.load()
    old = {}
    for n in KNOBS:
        v = ctypes.c_int(0)
        _lib.check(lib.papc_knob_get(n.encode(), ctypes.byref(v)), "papc_knob_get")
        old[n] = v.value

    def set_(name, value):
        assert name in old
        _lib.check(lib.papc_knob_set(name.encode(), int(value)), "papc_knob_set")

    yield set_
    for n, v in old.items():
        _lib.check(lib.papc_knob_set(n.encode(), v), "papc_knob_set")


def dev_(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def full(shape, value, dev, dtype=torch.float32):
    return torch.full(shape, value, device=dev, dtype=dtype)


def bits(x):
    return (np.asarray(x, F32) + F32(0)).view(np.int32)          # (-0 + 0 = +0: the two zeros are one value)


class Tally:
    """per test: outputs compared / differing, printed as the record the docstring quotes"""

    def __init__(self, family):
        self.family, self.n, self.bad, self.runs, self.msgs = family, 0, 0, 0, []

    def add(self, got, want, what):
        got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
        assert got.shape == want.shape, (what, got.shape, want.shape)
        d = bits(got) != bits(want)
        self.n += d.size
        self.runs += 1
        if d.any():
            i = tuple(int(v) for v in np.argwhere(d)[0])
            self.bad += int(d.sum())
            self.msgs.append("%s: %d of %d differ, first at %s: got %r (0x%08x) want %r (0x%08x)" % (what, d.sum(), d.size, i, float(got[i]),
                                                                                                  int(bits(got)[i]) & 0xffffffff, float(want[i]), int(bits(want)[i]) & 0xffffffff))

    def done(self):
        print("[exact] %s: %d of %d outputs differ (%d launches)" % (self.family, self.bad, self.n, self.runs))
        assert not self.msgs, "\n".join(self.msgs[:12])


def identity_bn(C, dev):
    """[6, C]: mean 0 | invstd 1 | scale 1 | shift | c1 0 | c2 0 -- shift 1 for a dY source (y = 0 is alive), 0 for a BN+ReLU operand"""
    return torch.tensor([0.0, 1.0, 1.0, 1.0, 0.0, 0.0], device=dev).view(6, 1).expand(6, C).contiguous()


def make_dy(dev, mode, C, y, dz=None, gout=None, argmax=None, K=0):
    cst = identity_bn(C, dev)
    d = BwdDy()
    d.dz_mode, d.K, d.y = mode, K, y.data_ptr()
    d.dz, d.gout, d.argmax = _lib.ptr(dz), _lib.ptr(gout), _lib.ptr(argmax)
    d.mean, d.invstd, d.scale, d.shift, d.c1, d.c2 = (cst[i].data_ptr() for i in range(6))
    return d, (cst, y, dz, gout, argmax)


# ---- tier 1: tiled forward (papc_mlp_gemm_f32) -----------------------------------------------------------------------------------
def run_forward(dev, a_mode, pr, ldx):
    lib = _lib.load()
    M, Cin = pr.A.shape
    Cout = pr.B.shape[0]
    x = torch.zeros(M, ldx, device=dev)
    x[:, :Cin] = dev_(pr.A, dev)
    w, bias = dev_(pr.B, dev), torch.zeros(Cout, device=dev)
    sc, sh = torch.ones(Cin + 3, device=dev), torch.zeros(Cin + 3, device=dev)
    y = full((M, Cout), float("nan"), dev)
    stats = torch.empty(lib.papc_mlp_gemm_parts(M), 2, Cout, device=dev)
    _lib.check(lib.papc_mlp_gemm_f32(a_mode, x.data_ptr(), ldx, None, sc.data_ptr(), sh.data_ptr(), w.data_ptr(), bias.data_ptr(), M, Cin, Cout, y.data_ptr(),
                                     stats.data_ptr(), None, _lib.stream_ptr()), "papc_mlp_gemm_f32")
    return y


TILE_FLAVOURS = ((0, 192, 0), (1, 192, 0), (0, 1, 0), (1, 1, 0), (0, 1, 4))      # (PAPC_GEMM_KB, PAPC_GEMM_MINWG, PAPC_GEMM_WAVES)


@gpu
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("cin", TILED_CIN)
@pytest.mark.parametrize("a_mode", [A_PLAIN, A_BNRELU])
def test_tiled_forward(dev, knob, a_mode, cin, f32):
    """gemm_kernel, forward: M = 200 is no multiple of 32, so stream_gemm_try declines (mlp_stream.hip:988) whatever the knobs say.
    ldx = Cin: the vector loader where Cin % 4 == 0; ldx = Cin + 1: the scalar one (fill_asrc: ldx % 4).  Tile flavours: k stages of 32 (two
    row tiles: kb2) and of 16 (PAPC_GEMM_KB=1); the 32-column tile <4,1,1,1> (two row tiles are under PAPC_GEMM_MINWG) and, with
    PAPC_GEMM_MINWG=1, the 64-column <2,2,2,1> and the 128-column tile on eight waves <2,4,2,1> and on four <2,2,2,2>"""
    knob("PAPC_GEMM_F32", f32)
    tally = Tally("tiled forward a_mode %d Cin %d f32 %d" % (a_mode, cin, f32))
    for cout in TILED_COUT:
        pr = single_term(TILED_M, cout, cin)
        for ldx in (cin, cin + 1) if cin % 4 == 0 else (cin, cin + 3):
            for kb, minwg, waves in TILE_FLAVOURS:
                knob("PAPC_GEMM_KB", kb), knob("PAPC_GEMM_MINWG", minwg), knob("PAPC_GEMM_WAVES", waves)
                tally.add(run_forward(dev, a_mode, pr, ldx), pr.expect, "Cout %d ldx %d kb %d minwg %d waves %d" % (cout, ldx, kb, minwg, waves))
    tally.done()


@gpu
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("xyz_first", [1, 0])
@pytest.mark.parametrize("D", GROUP_D)
def test_tiled_forward_grouped(dev, knob, D, xyz_first, f32):
    """A_GROUP: rows gathered through a permutation (one cloud, M points, 25 groups of 8), new_xyz = 0; D = 16 is the vector loader, D = 5 the
    scalar one (fill_asrc: D % 4); both column orders of the caller's weight (gk())"""
    lib = _lib.load()
    knob("PAPC_GEMM_F32", f32)
    M, Cin, K = TILED_M, D + 3, 8
    tally = Tally("tiled forward A_GROUP D %d xyz_first %d f32 %d" % (D, xyz_first, f32))
    perm = torch.from_numpy(((37 * np.arange(M) + 11) % M).astype(np.int32)).to(dev)
    for cout in TILED_COUT:
        pr = single_term(M, cout, Cin)
        A = dev_(pr.A, dev)
        xyz, feats = torch.zeros(1, M, 3, device=dev), torch.zeros(1, M, D, device=dev)
        xyz[0, perm.long()] = A[:, :3] if xyz_first else A[:, D:]
        feats[0, perm.long()] = A[:, 3:] if xyz_first else A[:, :D]
        new_xyz = torch.zeros(1, M // K, 3, device=dev)
        g = GroupSrc()
        g.xyz, g.sb, g.sn, g.sc, g.new_xyz, g.feats, g.idx = xyz.data_ptr(), 3 * M, 3, 1, new_xyz.data_ptr(), feats.data_ptr(), perm.data_ptr()
        g.N, g.S, g.K, g.D, g.xyz_first = M, M // K, K, D, xyz_first
        w, bias = dev_(pr.B, dev), torch.zeros(cout, device=dev)
        for kb, minwg, waves in TILE_FLAVOURS:
            knob("PAPC_GEMM_KB", kb), knob("PAPC_GEMM_MINWG", minwg), knob("PAPC_GEMM_WAVES", waves)
            y = full((M, cout), float("nan"), dev)
            stats = torch.empty(lib.papc_mlp_gemm_parts(M), 2, cout, device=dev)
            _lib.check(lib.papc_mlp_gemm_f32(A_GROUP, None, 0, ctypes.byref(g), None, None, w.data_ptr(), bias.data_ptr(), M, Cin, cout, y.data_ptr(),
                                             stats.data_ptr(), None, _lib.stream_ptr()), "papc_mlp_gemm_f32")
            tally.add(y, pr.expect, "Cout %d kb %d minwg %d waves %d" % (cout, kb, minwg, waves))
    tally.done()


# ---- tier 1: row-streaming forward (papc_mlp_gemm_rows_f32 / _rows_w_f32) --------------------------------------------------------
@gpu
@pytest.mark.parametrize("asm", [1, 0])
@pytest.mark.parametrize("cin,cout", STREAM_SHAPES)
@pytest.mark.parametrize("a_mode", [A_PLAIN, A_BNRELU])
def test_streaming_forward(dev, knob, a_mode, cin, cout, asm):
    """stream_kernel, forward, on a capacity of 65 536 rows of which rows_dev = 256 exist.  A device-side row count has no tiled flavour
    (mlp_gemm.hip:918-921: PAPC_E_UNSUPPORTED), so a call that returns has run the row-streaming kernel.  Rows behind the count stay untouched"""
    lib = _lib.load()
    knob("PAPC_STREAM", 1), knob("PAPC_STREAM_MINTILES", 1), knob("PAPC_STREAM_ASM", asm), knob("PAPC_GEMM_F32", 0)
    ragged = cin == 196
    if ragged and (a_mode == A_PLAIN or not asm):
        # stream_pick has the 196-channel input for BN+ReLU operands only (mlp_stream.hip:943) and stream_go builds ragged k on the asm ring only (:918)
        rows = dev_(np.array([ROWS_DEV], np.int32), dev)
        x, w, y = torch.zeros(CAPACITY, cin, device=dev), torch.zeros(cout, cin, device=dev), torch.zeros(CAPACITY, cout, device=dev)
        one = torch.ones(cin, device=dev)
        rc = lib.papc_mlp_gemm_rows_f32(a_mode, x.data_ptr(), cin, None, one.data_ptr(), one.data_ptr(), w.data_ptr(), None, CAPACITY, cin, cout, y.data_ptr(),
                                        None, None, rows.data_ptr(), _lib.stream_ptr())
        assert rc == -2, "a flavour that is not built must be refused (PAPC_E_UNSUPPORTED), got %d" % rc
        return
    pr = single_term(ROWS_DEV, cout, cin)
    tally = Tally("row-streaming forward a_mode %d %d -> %d asm %d" % (a_mode, cin, cout, asm))
    x = torch.zeros(CAPACITY, cin, device=dev)
    x[:ROWS_DEV] = dev_(pr.A, dev)
    w, bias = dev_(pr.B, dev), torch.zeros(cout, device=dev)
    sc, sh = torch.ones(cin, device=dev), torch.zeros(cin, device=dev)
    rows, wrow = dev_(np.array([ROWS_DEV], np.int32), dev), torch.ones(CAPACITY, device=dev)
    stats = torch.empty(lib.papc_mlp_gemm_parts(CAPACITY), 2, cout, device=dev)
    for nw12 in (1, 0):
        for weighted in ((0,) if ragged else (0, 1)):          # (weighted statistics are not built for the ragged flavours: mlp_stream.hip:940)
            knob("PAPC_STREAM_NW12", nw12)
            y = full((CAPACITY, cout), float("nan"), dev)
            if weighted:
                rc = lib.papc_mlp_gemm_rows_w_f32(a_mode, x.data_ptr(), cin, None, sc.data_ptr(), sh.data_ptr(), w.data_ptr(), bias.data_ptr(), CAPACITY, cin, cout,
                                                  y.data_ptr(), stats.data_ptr(), None, rows.data_ptr(), wrow.data_ptr(), _lib.stream_ptr())
            else:
                rc = lib.papc_mlp_gemm_rows_f32(a_mode, x.data_ptr(), cin, None, sc.data_ptr(), sh.data_ptr(), w.data_ptr(), bias.data_ptr(), CAPACITY, cin, cout,
                                                y.data_ptr(), stats.data_ptr(), None, rows.data_ptr(), _lib.stream_ptr())
            _lib.check(rc, "papc_mlp_gemm_rows%s_f32" % ("_w" if weighted else ""))
            tally.add(y[:ROWS_DEV], pr.expect, "nw12 %d weighted %d" % (nw12, weighted))
            assert bool(torch.isnan(y[ROWS_DEV:ROWS_DEV + 512]).all()), "rows behind the device-side count were written"
    tally.done()


# ---- tier 1: dX (papc_mlp_bwd_dx_f32) --------------------------------------------------------------------------------------------
def run_dx(dev, mode, pr, M, red, km=None, K=DX_K, cap=None, compact=None, psel=False):
    """dX [M, Cin] = dY [M, Cout] wt^T with dY = pr.A through the identity BatchNorm backward; ``cap``: the buffers' row capacity (a compacted
    stack: rows_dev = M of them exist, wrow = 1, seg_grp = row / 8 / (K / 8), argmax in absolute rows)"""
    lib = _lib.load()
    Cout, Cin = pr.A.shape[1], pr.B.shape[0]
    R = cap or M
    y = torch.zeros(R, Cout, device=dev)
    keep = []
    if mode == DZ_DENSE:
        dz = torch.zeros(R, Cout, device=dev)
        dz[:M] = dev_(pr.A, dev)
        dy, k2 = make_dy(dev, DZ_DENSE, Cout, y, dz=dz)
    else:
        G = M // K
        gout, argmax = np.zeros((R // K, Cout), F32), np.full((R // K, Cout), -1, np.int32)
        live = np.flatnonzero(km >= 0)
        gout[live // K, km[live]] = pr.A[live, km[live]]
        argmax[live // K, km[live]] = live if compact else live % K
        assert G * K == M
        gout_t = dev_(gout, dev)
        dy, k2 = make_dy(dev, DZ_MAX, Cout, y, gout=gout_t, argmax=dev_(argmax, dev), K=K)
        if psel:
            dy.psel = gout_t.data_ptr()         # scale = 1 and every selected value alive: psel = scale p = gout
    keep.append(k2)
    if compact:
        wrow, rows = torch.ones(R, device=dev), dev_(np.array([M], np.int32), dev)
        seg = dev_((np.arange(R // 8) // (K // 8)).astype(np.int32), dev)
        dy.wrow, dy.rows_dev, dy.seg_grp = wrow.data_ptr(), rows.data_ptr(), seg.data_ptr()
        keep.append((wrow, rows, seg))
    wt = dev_(pr.B, dev)
    dx = full((R, Cin), float("nan"), dev)
    nr = None
    if red:
        yp, cst = torch.zeros(R, Cin, device=dev), identity_bn(Cin, dev)
        part = torch.empty(lib.papc_mlp_gemm_parts(R), 2, Cin, device=dev)
        nr = BwdRed(yp.data_ptr(), cst[0].data_ptr(), cst[1].data_ptr(), cst[2].data_ptr(), cst[3].data_ptr(), part.data_ptr(), 0)
        keep.append((yp, cst, part))
    _lib.check(lib.papc_mlp_bwd_dx_f32(ctypes.byref(dy), wt.data_ptr(), R, Cin, Cout, dx.data_ptr(), None, ctypes.byref(nr) if red else None, _lib.stream_ptr()),
               "papc_mlp_bwd_dx_f32")
    torch.cuda.synchronize()
    return dx


@gpu
@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("cout,cin", DX_TILED)
@pytest.mark.parametrize("mode", [DZ_DENSE, DZ_MAX])
def test_tiled_dx(dev, knob, mode, cout, cin, f32):
    """gemm_kernel, A_DY_DENSE / A_DY_MAX: PAPC_STREAM=0 keeps the row-streaming kernel out (mlp_stream.hip:987).  With and without the fused
    reduction of the layer below (EPI_STORE_RED / EPI_STORE), the column-lane epilogue and the transposed one (PAPC_GEMM_TL: the MFMA operands
    swapped, mlp_gemm.hip:309), the tile flavours of the forward; (21, 13) is the scalar loader"""
    knob("PAPC_STREAM", 0), knob("PAPC_GEMM_F32", f32)
    km = max_rows(DX_M, cout, DX_K) if mode == DZ_MAX else None
    pr = single_term(DX_M, cin, cout, sign_a=True, km=km)
    tally = Tally("tiled dX mode %d %d -> %d f32 %d" % (mode, cout, cin, f32))
    for red in (False, True):
        for tl in (0, 1):
            for kb, minwg, waves in TILE_FLAVOURS:
                knob("PAPC_GEMM_TL", tl), knob("PAPC_GEMM_KB", kb), knob("PAPC_GEMM_MINWG", minwg), knob("PAPC_GEMM_WAVES", waves)
                tally.add(run_dx(dev, mode, pr, DX_M, red, km), pr.expect, "red %d tl %d kb %d minwg %d waves %d" % (red, tl, kb, minwg, waves))
    tally.done()


@gpu
@pytest.mark.parametrize("asm", [1, 0])
@pytest.mark.parametrize("cout,cin", DX_STREAM)
@pytest.mark.parametrize("mode", [DZ_DENSE, DZ_MAX])
def test_streaming_dx(dev, knob, mode, cout, cin, asm):
    """the dX dispatch with PAPC_STREAM=1 and PAPC_STREAM_MINTILES=1 on M = 256 rows: stream_kernel where stream_pick has the flavour
    (A_DY_DENSE / A_DY_MAX with the fused reduction; A_DY_DENSE alone for 64 and 128 channels of Cout), the tiled kernel elsewhere -- the same
    expectation either way.  PAPC_STREAM_NW12 both ways (the twelve-wave flavour: A_DY_MAX, Cout = 256, Cin = 64)"""
    knob("PAPC_STREAM", 1), knob("PAPC_STREAM_MINTILES", 1), knob("PAPC_STREAM_ASM", asm), knob("PAPC_GEMM_F32", 0)
    M = ROWS_DEV
    km = max_rows(M, cout, DX_K) if mode == DZ_MAX else None
    pr = single_term(M, cin, cout, sign_a=True, km=km)
    tally = Tally("streaming dX mode %d %d -> %d asm %d" % (mode, cout, cin, asm))
    for red in (True, False):
        for nw12 in (1, 0):
            knob("PAPC_STREAM_NW12", nw12)
            tally.add(run_dx(dev, mode, pr, M, red, km), pr.expect, "red %d nw12 %d" % (red, nw12))
    tally.done()


@gpu
@pytest.mark.parametrize("flavour", ["dense", "max", "max_psel"])
def test_compacted_dx(dev, knob, flavour):
    """the CP flavours of stream_kernel (mlp_stream.hip:928-935): 128 -> 128 dense and 256 -> 128 under the max, from gout and from psel, on a capacity
    of 65 536 rows of which rows_dev = 256 exist, wrow = 1, groups of 32 rows given by seg_grp, argmax in absolute rows.  A compacted dY source
    has no other kernel (mlp_gemm.hip:918-921)"""
    knob("PAPC_STREAM", 1), knob("PAPC_STREAM_MINTILES", 1), knob("PAPC_STREAM_ASM", 1), knob("PAPC_GEMM_F32", 0)
    M, cin = ROWS_DEV, 128
    cout, mode = (128, DZ_DENSE) if flavour == "dense" else (256, DZ_MAX)
    km = max_rows(M, cout, DX_K) if mode == DZ_MAX else None
    pr = single_term(M, cin, cout, sign_a=True, km=km)
    tally = Tally("compacted dX " + flavour)
    dx = run_dx(dev, mode, pr, M, True, km, cap=CAPACITY, compact=True, psel=flavour == "max_psel")
    tally.add(dx[:M], pr.expect, flavour)
    assert bool(torch.isnan(dx[M:M + 512]).all()), "rows behind the device-side count were written"
    tally.done()


# ---- tier 1: dW (papc_mlp_bwd_dw_f32, papc_mlp_bwd_dw_max_f32) -------------------------------------------------------------------
def run_dw(dev, pr, a_mode, mode, M, Cin, Cout, K, rpc=64):
    lib = _lib.load()
    y = torch.zeros(M, Cout, device=dev)
    if mode == DZ_DENSE:
        dy, keep = make_dy(dev, DZ_DENSE, Cout, y, dz=dev_(pr.dY, dev))
    else:
        dy, keep = make_dy(dev, DZ_MAX, Cout, y, gout=dev_(pr.gout, dev), argmax=dev_(pr.argmax, dev), K=K)
    x = dev_(pr.X, dev)
    sc, sh = torch.ones(Cin, device=dev), torch.zeros(Cin, device=dev)
    nch = (M + rpc - 1) // rpc
    n = Cout * Cin
    part = full((nch, n + Cout), float("nan"), dev)
    _lib.check(lib.papc_mlp_bwd_dw_f32(ctypes.byref(dy), a_mode, x.data_ptr(), Cin, None, sc.data_ptr(), sh.data_ptr(), M, Cin, Cout, rpc, part.data_ptr(),
                                       part.data_ptr() + 4 * n, n + Cout, _lib.stream_ptr()), "papc_mlp_bwd_dw_f32")
    # the chunks' partials folded by the library (each output has its terms in some chunks and exact zeros in the others)
    out = full((n + Cout,), float("nan"), dev)
    _lib.check(lib.papc_reduce_partials_f32(part.data_ptr(), nch, n + Cout, out.data_ptr(), 0, _lib.stream_ptr()), "papc_reduce_partials_f32")
    torch.cuda.synchronize()
    return out[:n].view(Cout, Cin)


DW_FLAVOURS = ((0, 1, 1, 1), (0, 0, 0, 1), (0, 0, 0, 0), (1, 1, 1, 1))      # (PAPC_DW_F32, PAPC_DW_ROWS, PAPC_DW_ROWSX, PAPC_DW_RS64)


@gpu
@pytest.mark.parametrize("cin,cout,a_mode,M,K", DW_CASES)
@pytest.mark.parametrize("mode", [DZ_DENSE, DZ_MAX])
def test_dw(dev, knob, mode, cin, cout, a_mode, M, K):
    """papc_mlp_bwd_dw_f32 in two row chunks (64 rows and a ragged rest) folded by papc_reduce_partials_f32: sums of 4, 2 and 1 equal terms whose
    rows lie in both chunks.  Kernel per case: launch_dw_v (mlp_dw.hip:1324-1381) -- M = 112 with a BN+ReLU input: dw_rowsx_kernel for
    128 -> 128 k and the ragged pairs, dw_rows_kernel for 64 -> 64 / 128; with PAPC_DW_ROWS = PAPC_DW_ROWSX = 0, a plain input or M = 100:
    dw_ws_kernel (64-row stages with PAPC_DW_RS64) where both widths are >= 64 and Cin % 4 == 0, dw_kernel (true-fp32 MFMA) elsewhere and
    under PAPC_DW_F32=1"""
    pr = dw_operands(M, cin, cout, K)
    tally = Tally("dW mode %d a_mode %d %d -> %d M %d" % (mode, a_mode, cin, cout, M))
    for f32, rows, rowsx, rs64 in DW_FLAVOURS:
        knob("PAPC_DW_F32", f32), knob("PAPC_DW_ROWS", rows), knob("PAPC_DW_ROWSX", rowsx), knob("PAPC_DW_RS64", rs64)
        tally.add(run_dw(dev, pr, a_mode, mode, M, cin, cout, K), pr.expect, "f32 %d rows %d rowsx %d rs64 %d" % (f32, rows, rowsx, rs64))
    tally.done()


@gpu
@pytest.mark.parametrize("case", ["classes", "gram"])
def test_dw_max_without_stored_output(dev, knob, case):
    """papc_mlp_bwd_dw_max_f32 (dw_rows_max_kernel, 64 -> 128, groups of 32): the chunk partials T = P'^T A | Gram | column sums are raw accumulators
    in the caller's workspace ([chunks][(Cout + 64) 64 + 64] floats first), folded here by papc_reduce_partials_f32.  "classes": T as sums of
    4, 2, 1, 1 equal terms over dense decoy rows; "gram": one non-zero input row, so that the Gram accumulator (mlp_dw.hip:1181) and the
    column sums are single terms too"""
    lib = _lib.load()
    knob("PAPC_STREAM", 1), knob("PAPC_STREAM_MINTILES", 1), knob("PAPC_STREAM_ASM", 1), knob("PAPC_STREAM_MAXCAT", 1), knob("PAPC_MAX_NOSTORE", 1)
    knob("PAPC_DW_ROWS", 1), knob("PAPC_DW_F32", 0), knob("PAPC_GEMM_F32", 0), knob("PAPC_GEMM_MINWG", 1)
    M, K, Cin, Cout = 256, 32, 64, 128
    assert lib.papc_mlp_max_nostore_ok(M, Cin, Cout, K) == 1
    tally = Tally("dW max without stored output, " + case)
    if case == "classes":
        pr = dw_operands(M, Cin, Cout, K)
        X, psel, argmax, checks = pr.X, pr.gout, pr.argmax, [("T", 0, Cout, pr.expect)]
    else:
        t, g, X, psel, argmax, xr = gram_operands(M, K, Cin, Cout)
        checks = [("T", 0, Cout, t.expect), ("Gram", Cout, Cin, g.expect), ("column sums", Cout + Cin, 1, xr.reshape(1, Cin))]
    n = (Cout + Cin) * Cin + Cin
    ws = full((lib.papc_mlp_bwd_dw_max_ws_floats(M, Cin, Cout),), float("nan"), dev)
    nch = (ws.numel() - 2 * n - 2) // n
    x, ps, am = dev_(X, dev), dev_(psel, dev), dev_(argmax, dev)
    sc, sh, zc, dw = torch.ones(Cin, device=dev), torch.zeros(Cin, device=dev), torch.zeros(Cout, device=dev), torch.empty(Cout, Cin, device=dev)
    w = torch.zeros(Cout, Cin, device=dev)
    _lib.check(lib.papc_mlp_bwd_dw_max_f32(ps.data_ptr(), am.data_ptr(), K, x.data_ptr(), sc.data_ptr(), sh.data_ptr(), w.data_ptr(), zc.data_ptr(), zc.data_ptr(),
                                           zc.data_ptr(), M, Cin, Cout, ws.data_ptr(), dw.data_ptr(), 0, _lib.stream_ptr()), "papc_mlp_bwd_dw_max_f32")
    out = full((n,), float("nan"), dev)
    _lib.check(lib.papc_reduce_partials_f32(ws.data_ptr(), nch, n, out.data_ptr(), 0, _lib.stream_ptr()), "papc_reduce_partials_f32")
    torch.cuda.synchronize()
    for what, r0, nr, want in checks:
        tally.add(out[r0 * Cin:(r0 + nr) * Cin].view(nr, Cin), want, what)
    tally.done()


# ---- tier 1: planes (papc_pg_*) --------------------------------------------------------------------------------------------------
def planes_buf(R, K, dev):
    return torch.zeros(_lib.load().papc_pg_planes_bytes(R, K), dtype=torch.uint8, device=dev)


def prep_rows(dev, x, transposed):
    """planes of x [M, C] (contraction over C), or planes_t: of x^T (contraction over M)"""
    M, C = x.shape
    a = smallm.PgPrep()
    a.mode, a.M, a.C, a.x, a.ldx = smallm.PLAIN, M, C, x.data_ptr(), C
    buf = planes_buf(C, M, dev) if transposed else planes_buf(M, C, dev)
    if transposed:
        a.planes_t = buf.data_ptr()
    else:
        a.planes = buf.data_ptr()
    _lib.check(_lib.load().papc_pg_prep_rows_f32(ctypes.byref(a), _lib.stream_ptr()), "papc_pg_prep_rows_f32")
    return buf


def prep_weights(dev, w):
    R, K = w.shape
    job = (smallm.PgWJob * 1)()
    buf = planes_buf(R, K, dev)
    job[0].src, job[0].row_stride, job[0].col_stride, job[0].R, job[0].K, job[0].planes = w.data_ptr(), K, 1, R, K, buf.data_ptr()
    _lib.check(_lib.load().papc_pg_prep_weights_f32(job, 1, _lib.stream_ptr()), "papc_pg_prep_weights_f32")
    return buf


def pg_product(a, b, R1, R2, K, c, split=1, stride=0):
    g = smallm.PgGemm()
    g.epi, g.a, g.b, g.R1, g.R2, g.K, g.c, g.ldc, g.split, g.split_stride, g.family = smallm.EPI_STORE, a.data_ptr(), b.data_ptr(), R1, R2, K, c.data_ptr(), R2, split, stride, 3
    return g


@gpu
@pytest.mark.parametrize("pipe", [1, 0])
@pytest.mark.parametrize("K", PG_K + (64,))
@pytest.mark.parametrize("R2", PG_R2)
def test_planes(dev, knob, R2, K, pipe):
    """papc_pg_prep_rows_f32 (PLAIN: planes, and planes_t of the transposed matrix where the contraction is a multiple of 32 -- K = 40 is not,
    K = 64 stands in) and papc_pg_prep_weights_f32 feed papc_pg_gemm_f32 (PAPC_PG_STORE; K = 40 and 64 are two k32 stages: split 1 and 2 +
    papc_pg_fold_f32) and papc_pg_gemm_group_f32 (two products in one grid).  PAPC_PG_PIPE=1 is the k16 ring (smallm.hip:489), 0 the k32 stage
    loop (:609), also on three stages (PAPC_PG_NS=3) and on 128-column tiles (PAPC_PG_NB=2)"""
    lib = _lib.load()
    knob("PAPC_PG_PIPE", pipe), knob("PAPC_PG_GROUP", 1)
    R1 = PG_R1
    pr = single_term(R1, R2, K)
    tally = Tally("planes %d x %d x %d pipe %d" % (R1, R2, K, pipe))
    A, B = dev_(pr.A, dev), dev_(pr.B, dev)
    pb = prep_weights(dev, B)
    sets = [("planes", prep_rows(dev, A, False))]
    if K % 32 == 0:
        sets.append(("planes_t", prep_rows(dev, A.t().contiguous(), True)))
    st = _lib.stream_ptr()
    for name, pa in sets:
        for nb, ns in ((0, 0), (2, 0), (0, 3)):
            knob("PAPC_PG_NB", nb), knob("PAPC_PG_NS", ns)
            c = full((R1, R2), float("nan"), dev)
            g = pg_product(pa, pb, R1, R2, K, c)
            _lib.check(lib.papc_pg_gemm_f32(ctypes.byref(g), st), "papc_pg_gemm_f32")
            tally.add(c, pr.expect, "%s nb %d ns %d" % (name, nb, ns))
            if K > 32:
                part, out = full((2, R1 * R2), float("nan"), dev), full((R1, R2), float("nan"), dev)
                g = pg_product(pa, pb, R1, R2, K, part, split=2, stride=R1 * R2)
                _lib.check(lib.papc_pg_gemm_f32(ctypes.byref(g), st), "papc_pg_gemm_f32 (split 2)")
                job = (smallm.PgFoldJob * 1)()
                job[0].partial, job[0].nsplit, job[0].stride, job[0].n, job[0].out, job[0].accumulate = part.data_ptr(), 2, R1 * R2, R1 * R2, out.data_ptr(), 0
                _lib.check(lib.papc_pg_fold_f32(job, 1, st), "papc_pg_fold_f32")
                tally.add(out, pr.expect, "%s nb %d ns %d split 2" % (name, nb, ns))
        knob("PAPC_PG_NB", 0), knob("PAPC_PG_NS", 0)
        # two products in one grid: this one and its mirror image B A^T
        pa2, pb2 = prep_weights(dev, A), pb
        c1, c2 = full((R1, R2), float("nan"), dev), full((R2, R1), float("nan"), dev)
        gs = (smallm.PgGemm * 2)(pg_product(pa, pb, R1, R2, K, c1), pg_product(pb2, pa2, R2, R1, K, c2))
        _lib.check(lib.papc_pg_gemm_group_f32(gs, 2, st), "papc_pg_gemm_group_f32")
        tally.add(c1, pr.expect, name + " grouped, first product")
        tally.add(c2, np.ascontiguousarray(pr.expect.T), name + " grouped, mirrored product")
    tally.done()


# ---- tier 2: the mfma_bf16x3() callers whose output is an image of the accumulator -----------------------------------------------
@gpu
@pytest.mark.parametrize("cp,cout", CCK_SHAPES)
def test_cloud_concat_k_forward(dev, cp, cout):
    """papc_cloud_concat_k_f32 (cloud_concat_k.hip:113): y = W_p x + c[b] with the cloud vector g = 0 and bias = 0, so c is an exact zero
    (an fmaf chain over zeros) whatever W_g holds, and y the accumulator"""
    lib = _lib.load()
    B, N, Cg = CCK_B, CCK_N, CCK_CG
    M = B * N
    pr = single_term(M, cout, cp)
    tally = Tally("cloud concat k forward %d -> %d" % (cp, cout))
    w = torch.zeros(cout, cp + Cg, device=dev)
    w[:, :cp] = dev_(pr.B, dev)
    w[:, cp:] = dev_(pr.B[:, :Cg], dev)             # (decoys: they multiply g = 0)
    x, g, bias = dev_(pr.A, dev), torch.zeros(B, Cg, device=dev), torch.zeros(cout, device=dev)
    y, cvec = full((M, cout), float("nan"), dev), full((B, cout), float("nan"), dev)
    stats = torch.empty(lib.papc_cloud_concat_k_parts(B, N), 2, cout, device=dev)
    _lib.check(lib.papc_cloud_concat_k_f32(x.data_ptr(), cp, g.data_ptr(), w.data_ptr(), bias.data_ptr(), B, N, cp, Cg, cout, y.data_ptr(), cvec.data_ptr(),
                                           stats.data_ptr(), _lib.stream_ptr()), "papc_cloud_concat_k_f32")
    tally.add(y, pr.expect, "y")
    tally.add(cvec, np.zeros((B, cout), F32), "c")
    tally.done()


@gpu
@pytest.mark.parametrize("cin,f", KD_SHAPES)
def test_kdconv_forward(dev, cin, f):
    """papc_kdconv_fwd_f32 (kd_step, kdlevel.h:50): positive operands and no bias, so the ReLU passes every product and the pooled output is
    the larger accumulator of its row pair -- an exact image of one of the two (which one: win, compared as well)"""
    lib = _lib.load()
    B, dim = KD_B, KD_DIM
    M = B * dim
    assert lib.papc_kdconv_ok(dim, cin, f) == 1
    pr = positive(single_term(M, 3 * f, cin))
    tally = Tally("kd conv forward %d -> 3 x %d" % (cin, f))
    sel = kd_select()
    k, p = kd_rows(sel)                                                                   # [B, dim]
    src = (np.arange(B)[:, None] * dim + p).reshape(-1)                                   # source row of every pre-pool row
    chan = 3 * np.arange(f)[None, :] + k.reshape(-1)[:, None]                             # its conv channel per feature
    pre = pr.expect[src[:, None], chan]                                                   # [M, F]
    assert (pre > 0).all()
    want, win = np.maximum(pre[0::2], pre[1::2]), (pre[1::2] > pre[0::2]).astype(np.uint8)
    x, w, sel_t = dev_(pr.A, dev), dev_(pr.B, dev), dev_(sel, dev)
    out, wn = full((M // 2, f), float("nan"), dev), full((M // 2, f), 7, dev, torch.uint8)
    _lib.check(lib.papc_kdconv_fwd_f32(x.data_ptr(), cin, sel_t.data_ptr(), dim, w.data_ptr(), None, B, dim, cin, f, out.data_ptr(), wn.data_ptr(),
                                       _lib.stream_ptr()), "papc_kdconv_fwd_f32")
    tally.add(out, want, "out")
    assert np.array_equal(wn.cpu().numpy(), win), "the pair's winner differs"
    tally.done()


@gpu
@pytest.mark.parametrize("which", [0, 5])
def test_voxconv1_forward(dev, which):
    """papc_voxconv1_fwd_f32 (vox_step, voxconv.hip:58, the one product of every voxconv kernel): voxels on a period-6 lattice, no bias -- y1 is the
    accumulator, one term per row at a tap that varies with the row (and with the cloud), or an exact zero"""
    lib = _lib.load()
    B, E = VOX_B, VOX_E
    assert lib.papc_voxconv_ok(E) == 1
    x, pr = vox_operands(which)
    tally = Tally("vox conv1 forward, pair %d" % which)
    M1 = pr.A.shape[0]
    xt, w1 = dev_(x.astype(F32), dev), dev_(pr.B, dev)
    y1 = full((M1, 32), float("nan"), dev)
    stats = torch.empty(lib.papc_voxconv_parts(B, E), 2, 32, device=dev)
    _lib.check(lib.papc_voxconv1_fwd_f32(xt.data_ptr(), w1.data_ptr(), None, B, E, y1.data_ptr(), stats.data_ptr(), _lib.stream_ptr()), "papc_voxconv1_fwd_f32")
    tally.add(y1, pr.expect, "y1")
    tally.done()


@gpu
@pytest.mark.parametrize("C", [64, 40])
def test_pfn_apply(dev, knob, C):
    """papc_pfn_apply_f32 under PAPC_PFN_MFMA=1 (pfn_apply_mfma_kernel, pfn.hip:404) and, against the same expectation, =0 (the lanes-are-channels
    fmaf chain): out = max over the rows of relu(1 * y + 0) is the one non-zero row's accumulator, single terms at k = 2, 3 and two equal terms at
    k = 0 + 7 and 1 + 8"""
    lib = _lib.load()
    P, T = PFN_P, PFN_T
    feat, nv, pr = pfn_operands(C)
    assert (pr.expect > 0).all()
    tally = Tally("pfn apply, %d channels" % C)
    f, n, co, w = dev_(feat, dev), dev_(nv, dev), torch.zeros(P, 4, device=dev, dtype=torch.int32), dev_(pr.B, dev)
    sc, sh = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    for mfma in (1, 0):
        knob("PAPC_PFN_MFMA", mfma)
        out = full((P, C), float("nan"), dev)
        _lib.check(lib.papc_pfn_apply_f32(f.data_ptr(), n.data_ptr(), co.data_ptr(), P, T, 1.0, 1.0, 0.0, 0.0, w.data_ptr(), C, sc.data_ptr(), sh.data_ptr(),
                                          out.data_ptr(), None, _lib.stream_ptr()), "papc_pfn_apply_f32")
        tally.add(out, pr.expect, "PAPC_PFN_MFMA=%d" % mfma)
    tally.done()
