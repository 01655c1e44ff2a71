// kdlevel.h -- what a kd-tree select-conv level is, written once for kdconv.hip (KD-Net levels: conv, ReLU, select, pair max) and kdbn.hip
// (KDUNet down levels: the same with a BatchNorm between the conv and the ReLU).
//
// For pre-pool row n of a cloud, s = sel[n] in {0, 1, 2}:  j = 3n + s,  k = j / dim (weight plane),  p = j % dim (source point): the source's
// two reshapes and its index arithmetic as they are (kdnet.py:21-30, kdunet.py:51-61).  Here: that index rule; the 16-wide
// bf16x3 k step; the forward accumulation of a wave's 32 rows x 32 features and the walk over its 16 row pairs; the sparse dX accumulation;
// the chunk loop of dW with its per-plane row sums and the partial row they are stored to; the Cin = 3 twins of the two backward bodies; the
// host checks of the entry points' arguments.  The families differ in what they hand in: the epilogue of a row pair (a functor), how dy is
// formed from the pooled gradient (a functor: KdDyPlain here, kdbn.hip's times r_c) and the number of row sums per plane (1: db; 2: dbeta and
// dgamma, the latter from the stored zhat).  The two Cin = 3 forwards round differently (kdconv.hip starts its fmaf chain from the bias,
// kdbn.hip from w0 x0 without one), so each keeps its chain and only the row lookup is shared.
#pragma once
#include "bf16x3.h"

namespace papc {

constexpr unsigned KD_ROW = 0x3fffffffu;
constexpr int KD_T = 256;        // threads of every level kernel (4 waves)
constexpr int KD_CH = 128;       // rows per dW chunk (MFMA kernel)
constexpr int KD_CH3 = 256;      // rows per dW chunk (Cin = 3 kernel)

__device__ __forceinline__ float4 kd_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ int kd_clamp_s(int s) { return min(max(s, 0), 2); }

// pre-pool row m of the flattened rows -> (plane k << 30) | flattened source row; k = 3 for a row past M.  A split value outside 0..2 is
// clamped, so it cannot address outside the buffers.
__device__ __forceinline__ unsigned kd_row_info(int m, int M, int dim, const int *__restrict__ sel, int64_t ss)
{
    if (m >= M) return 3u << 30;
    const int b = m / dim, n = m - b * dim;
    const int j = 3 * n + kd_clamp_s(sel[(int64_t)b * ss + n]);
    const int k = (j >= dim) + (j >= 2 * dim);
    return ((unsigned)k << 30) | (unsigned)(b * dim + j - k * dim);
}

// the row of cloud b that source point p feeds through plane q, if any: 3n + s = p + q dim with s = sel[n]
__device__ __forceinline__ bool kd_fed_row(int b, int p, int q, int dim, const int *__restrict__ sel, int64_t ss, int &n)
{
    const int t = p + q * dim;
    n = t / 3;
    return kd_clamp_s(sel[(int64_t)b * ss + n]) == t - 3 * n;
}

// the 16-wide k step both operands of which are 8 consecutive floats per lane
__device__ __forceinline__ floatx16 kd_step(const float (&av)[8], const float (&bv)[8], floatx16 acc)
{
    bf16x8 ap[3], bp[3];
    split8(av, ap);
    split8(bv, bp);
    return mfma_bf16x3(ap, bp, acc);
}

__device__ __forceinline__ void kd_ld8(const float *p, float (&v)[8])
{
    const float4 a = kd_ld4(p), b = kd_ld4(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// dy of a selected winner with out > 0 from the pooled gradient g; c = 3f + q is its conv channel
struct KdDyPlain {
    __device__ __forceinline__ float operator()(float g, int) const { return g; }
};

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// wave: rows m0 .. m0 + 31, feature f = 32 fb + r per lane.  The points lie on the 32x32 accumulator's ROW axis (row = (reg & 3) + 8 (reg >> 2)
// + 4 (lane >> 5)), so both rows of a pair are registers of one lane and the pool needs no shuffle.  The wave loops over the planes present
// in its tile (a ballot); rows of another plane enter as zero A rows (their loads are skipped), so a row's accumulator receives its own
// plane's products and exact zeros.  A[row r][c] = x[source row of r][c] where r is of the plane at hand, B[c][col r] = W[3f + q][c]: both are
// 8 consecutive floats per lane and 16-wide k step, straight from global memory.  Returns w . x (no bias); k = the plane of row m0 + r.
__device__ __forceinline__ floatx16 kd_fwd_acc(const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss,
                                               const float *__restrict__ w, int M, int dim, int Cin, int m0, int f, int &k)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const unsigned info = kd_row_info(m0 + r, M, dim, sel, ss);
    k = (int)(info >> 30);
    const float *xr = x + (int64_t)(info & KD_ROW) * ldx + 8 * h;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int q = 0; q < 3; ++q) {
        if (__ballot(k == q) == 0) continue;            // (wave-uniform)
        const bool mine = k == q;
        const float *wr = w + (int64_t)(3 * f + q) * Cin + 8 * h;
        for (int c1 = 0; c1 < Cin; c1 += 32)           // (Cin is a multiple of 32: two k steps' loads in flight)
#pragma unroll
        for (int c0 = c1; c0 < c1 + 32; c0 += 16) {
            float av[8], bv[8];
            if (mine) kd_ld8(xr + c0, av);
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j) av[j] = 0.f;
            }
            kd_ld8(wr + c0, bv);
            acc = kd_step(av, bv, acc);
        }
    }
    return acc;
}

// the 16 row pairs of a forward accumulator: pair(acc of the even row, its plane, acc of the odd row, its plane, the pooled element's offset)
template <class Pair>
__device__ __forceinline__ void kd_fwd_pairs(const floatx16 &acc, int k, int m0, int M, int F, int f, Pair pair)
{
    const int h = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int row = 8 * g + 4 * h + 2 * t;      // lanes 0..31 hold the planes of rows 0..31
            const int k0 = __shfl(k, row), k1 = __shfl(k, row + 1);
            const int m = m0 + row;
            if (m < M)                                  // (M is even: row m + 1 exists)
                pair(acc[4 * g + 2 * t], k0, acc[4 * g + 2 * t + 1], k1, (int64_t)(m >> 1) * F + f);
        }
}

// Cin = 3 forward: pre-pool row m of feature f -> its conv channel o = 3f + k, the source row and the channel's three weights
__device__ __forceinline__ int kd_fwd3_row(int m, int M, int dim, const int *__restrict__ sel, int64_t ss, const float *__restrict__ x, int64_t ldx,
                                           const float *__restrict__ w, int f, const float *&xr, const float *&wr)
{
    const unsigned info = kd_row_info(m, M, dim, sel, ss);
    const int o = 3 * f + (int)(info >> 30);
    xr = x + (int64_t)(info & KD_ROW) * ldx;
    wr = w + (int64_t)o * 3;
    return o;
}

// ---- backward: dX -------------------------------------------------------------------------------------------------------------------
// dy[n, f] = dy(gout[n / 2, f]) where row n won its pair and out > 0, else 0 (winner byte: 0 = the even row, also on an exact tie).  Source
// point p feeds the rows with 3n + s = p + q dim, q = 0, 1, 2 (plane q) -- at most one row per q; the sparse term of dX[p] is
// sum_q dy[n_q] . W_plane q, accumulated in that order; points that feed no row get exact zeros.
// wave: source rows m0 .. m0 + 31, input channels 32 cb .. + 31.  A[row r][f] = dy[row fed by r through plane q][f] (8 consecutive f of one
// pooled row: gout, out and the winner bytes), B[f][col r] = W[3f + q][32 cb + r].
template <class Dy>
__device__ __forceinline__ floatx16 kd_dx_acc(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                              const int *__restrict__ sel, int64_t ss, const float *__restrict__ w, int M, int dim, int Cin, int F, int m0,
                                              int cb, Dy dy)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int m = m0 + r;
    const bool live = m < M;
    const int b = live ? m / dim : 0, p = live ? m - b * dim : 0;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int q = 0; q < 3; ++q) {
        int n = 0;
        const bool v = live && kd_fed_row(b, p, q, dim, sel, ss, n);
        if (__ballot(v) == 0) continue;
        const int64_t at = (((int64_t)b * dim + n) >> 1) * F + 8 * h;      // (b dim is even)
        const unsigned par = (unsigned)(n & 1);
        const float *wq = w + (int64_t)(3 * 8 * h + q) * Cin + cb * 32 + r;
        for (int f1 = 0; f1 < F; f1 += 32)             // (F is a multiple of 32: two k steps' loads in flight)
#pragma unroll
        for (int f0 = f1; f0 < f1 + 32; f0 += 16) {
            float av[8], bv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) bv[j] = wq[(int64_t)3 * (f0 + j) * Cin];
            if (v) {
                float g[8], o[8];
                kd_ld8(gout + at + f0, g);
                kd_ld8(outv + at + f0, o);
                const uint2 wb = *reinterpret_cast<const uint2 *>(win + at + f0);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned wj = ((j < 4 ? wb.x : wb.y) >> (8 * (j & 3))) & 0xffu;
                    av[j] = (o[j] > 0.f && wj == par) ? dy(g[j], 3 * (8 * h + f0 + j) + q) : 0.f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) av[j] = 0.f;
            }
            acc = kd_step(av, bv, acc);
        }
    }
    return acc;
}

// Cin = 3: thread = source row m; the sparse term of dX[m] is added to a[0..2]
template <class Dy>
__device__ __forceinline__ void kd_dx3_acc(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                           const int *__restrict__ sel, int64_t ss, const float *__restrict__ w, int m, int dim, int F, float (&a)[3], Dy dy)
{
    const int b = m / dim, p = m - b * dim;
    for (int q = 0; q < 3; ++q) {
        int n;
        if (!kd_fed_row(b, p, q, dim, sel, ss, n)) continue;
        const int64_t at = (((int64_t)b * dim + n) >> 1) * F;
        const unsigned par = (unsigned)(n & 1);
        for (int f = 0; f < F; ++f) {
            const float d = (outv[at + f] > 0.f && win[at + f] == par) ? dy(gout[at + f], 3 * f + q) : 0.f;
            const float *wr = w + (int64_t)(3 * f + q) * 3;
            a[0] = fmaf(d, wr[0], a[0]);
            a[1] = fmaf(d, wr[1], a[1]);
            a[2] = fmaf(d, wr[2], a[2]);
        }
    }
}

// ---- backward: dW and the row sums ----------------------------------------------------------------------------------------------------
// With g[n, f] = gout[n / 2, f] where row n won its pair and out > 0, else 0: per plane q the sums over the chunk's rows n of plane q of
// g[n, f] x[source row of n] (dW), of g[n, f] (sum 0) and, for NS = 2, of g[n, f] zh[n / 2, f] (sum 1).
// chunk = rows r0 .. r0 + 127; wave = one 32 x 32 block (features 32 fb .. , input channels 32 cb ..) of each of the three planes.
// A[row r = feature][n] = g[n][32 fb + r] for the rows n of plane q, B[n][col r] = x[source row of n][32 cb + r].  A lane's sums cover its
// half of each k step's rows; kd_dw_store adds the two halves.
template <int NS>
__device__ __forceinline__ void kd_dw_acc(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                          const float *__restrict__ zh, const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss,
                                          int M, int dim, int F, int r0, int f, int c, floatx16 (&acc)[3], float (&sums)[NS][3])
{
    static_assert(NS == 1 || NS == 2, "row sums per plane: g, or g and g zhat");
    const int lane = threadIdx.x & 63, h = lane >> 5;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) sums[s][q] = 0.f;
    }
    for (int ks = 0; ks < KD_CH / 16; ++ks) {
        const int mb = r0 + ks * 16;
        if (mb >= M) break;                                        // (wave-uniform)
        const unsigned info = kd_row_info(mb + (lane & 15), M, dim, sel, ss);     // the 16 rows of this k step, four times over
        const int kl = (int)(info >> 30);
        float dyv[8], zv[8], bv[8];
        int kj[8];
#pragma unroll
        for (int t = 0; t < 4; ++t) {                              // rows mb + 8h + 2t, + 1 = pooled row (mb + 8h) / 2 + t
            const int mr = mb + 8 * h + 2 * t;
            float g = 0.f, z = 0.f;
            unsigned wb = 0;
            if (mr < M) {
                const int64_t at = (int64_t)(mr >> 1) * F + f;
                g = outv[at] > 0.f ? gout[at] : 0.f;
                if (NS == 2) z = zh[at];
                wb = win[at];
            }
            dyv[2 * t] = wb == 0 ? g : 0.f;
            dyv[2 * t + 1] = wb == 0 ? 0.f : g;
            zv[2 * t] = zv[2 * t + 1] = z;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned inf = (unsigned)__shfl((int)info, 8 * h + j);
            kj[j] = (int)(inf >> 30);
            bv[j] = kj[j] < 3 ? x[(int64_t)(inf & KD_ROW) * ldx + c] : 0.f;
        }
        bf16x8 bp[3];
        split8(bv, bp);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (__ballot(kl == q) == 0) continue;
            float am[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) am[j] = kj[j] == q ? dyv[j] : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                sums[0][q] += am[j];
                if (NS == 2) sums[1][q] = fmaf(am[j], zv[j], sums[1][q]);
            }
            bf16x8 ap[3];
            split8(am, ap);
            acc[q] = mfma_bf16x3(ap, bp, acc[q]);
        }
    }
}

// the chunk's partial row pt: dW [3F, Cin], then sum 0 [3F], then sum 1 [3F]
template <int NS>
__device__ __forceinline__ void kd_dw_store(const floatx16 (&acc)[3], const float (&sums)[NS][3], float *__restrict__ pt, int Cin, int F, int fb, int cb)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int fr = fb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            pt[(int64_t)(3 * fr + q) * Cin + cb * 32 + r] = acc[q][i];
        }
        float tot[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) tot[s] = sums[s][q] + __shfl_xor(sums[s][q], 32);        // the two row halves of the lane pair
        if (cb == 0 && h == 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) pt[(int64_t)3 * F * Cin + (int64_t)s * 3 * F + 3 * (fb * 32 + r) + q] = tot[s];
        }
    }
}

// Cin = 3: chunk = pooled rows om0 .. om0 + 127 (256 rows); workgroup = 32 features at f0 x 8 slices of the chunk's pooled rows.  Only the
// winner of a pair carries a gradient.  Per plane 3 + NS sums (dW's three columns, then the row sums); the slices are added in slice order and
// stored to the partial row pt in kd_dw_store's layout.  Every thread of the workgroup calls.
template <int NS>
__device__ __forceinline__ void kd_dw3_chunk(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                             const float *__restrict__ zh, const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss,
                                             int M, int dim, int F, int om0, int f0, float (&red)[8][3 * (3 + NS)][32], float *__restrict__ pt)
{
    static_assert(NS == 1 || NS == 2, "row sums per plane: g, or g and g zhat");
    constexpr int NA = 3 + NS;
    const int fl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int f = f0 + fl;
    float a[3 * NA];
#pragma unroll
    for (int i = 0; i < 3 * NA; ++i) a[i] = 0.f;
    for (int i = sl; i < KD_CH3 / 2; i += 8) {
        const int om = om0 + i;
        if (2 * om >= M) break;
        const int64_t at = (int64_t)om * F + f;
        const float g = outv[at] > 0.f ? gout[at] : 0.f, z = NS == 2 ? zh[at] : 0.f;
        const unsigned info = kd_row_info(2 * om + (win[at] ? 1 : 0), M, dim, sel, ss);
        const int k = (int)(info >> 30);
        const float *xr = x + (int64_t)(info & KD_ROW) * ldx;
        const float x0 = xr[0], x1 = xr[1], x2 = xr[2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float d = k == q ? g : 0.f;
            a[NA * q] = fmaf(d, x0, a[NA * q]);
            a[NA * q + 1] = fmaf(d, x1, a[NA * q + 1]);
            a[NA * q + 2] = fmaf(d, x2, a[NA * q + 2]);
            a[NA * q + 3] += d;
            if (NS == 2) a[NA * q + 4] = fmaf(d, z, a[NA * q + 4]);
        }
    }
#pragma unroll
    for (int i = 0; i < 3 * NA; ++i) red[sl][i][fl] = a[i];
    __syncthreads();
    if (sl != 0) return;
#pragma unroll
    for (int i = 0; i < 3 * NA; ++i) {
        float s = a[i];
#pragma unroll
        for (int g = 1; g < 8; ++g) s += red[g][i][fl];
        const int q = i / NA, c = i - NA * q;
        if (c < 3) pt[(int64_t)(3 * f + q) * 3 + c] = s;
        else pt[(int64_t)3 * F * 3 + (int64_t)(c - 3) * 3 * F + 3 * f + q] = s;
    }
}

// ---- host: the entry points' arguments (who = the entry point's name, the prefix of every message) --------------------------------------
static bool kd_level_ok(int dim, int Cin, int F, int Fmax)
{
    return dim >= 2 && dim % 2 == 0 && (Cin == 3 || (Cin >= 32 && Cin <= 512 && Cin % 32 == 0)) && F >= 32 && F <= Fmax && F % 32 == 0;
}

static int kd_level_shape_ok(const char *who, int B, int dim, int Cin, int F, int Fmax)
{
    PAPC_REQUIRE(dim >= 2 && dim % 2 == 0, PAPC_E_UNSUPPORTED, "%s: dim=%d (points per cloud: even, >= 2)", who, dim);
    PAPC_REQUIRE(Cin == 3 || (Cin >= 32 && Cin <= 512 && Cin % 32 == 0), PAPC_E_UNSUPPORTED, "%s: Cin=%d (3, or a multiple of 32 up to 512)", who, Cin);
    PAPC_REQUIRE(F >= 32 && F <= Fmax && F % 32 == 0, PAPC_E_UNSUPPORTED, "%s: F=%d (a multiple of 32 up to %d)", who, F, Fmax);
    PAPC_REQUIRE(B >= 1 && (int64_t)B * dim <= ((int64_t)1 << 28), PAPC_E_INVALID, "%s: B=%d dim=%d (B >= 1, B * dim <= 2^28)", who, B, dim);
    return PAPC_OK;
}

static int64_t kd_level_chunks(int64_t M, int Cin) { return cdiv(M, Cin == 3 ? KD_CH3 : KD_CH); }

// the forward's strides and alignment
static int kd_level_fwd_args_ok(const char *who, const float *x, int64_t ldx, int64_t sel_stride, const float *w, int dim, int Cin)
{
    PAPC_REQUIRE(ldx >= Cin && (sel_stride == 0 || sel_stride >= dim), PAPC_E_INVALID, "%s: ldx=%lld < Cin or sel_stride=%lld (0 or >= dim)", who,
                 (long long)ldx, (long long)sel_stride);
    PAPC_REQUIRE(Cin == 3 || (ldx % 4 == 0 && aligned16(x) && aligned16(w)), PAPC_E_INVALID, "%s: x and w must be 16-byte aligned, ldx=%lld a multiple of 4",
                 who, (long long)ldx);
    return PAPC_OK;
}

// the backward's strides, alignment and workspace.  more_aligned: what a family's kernels read by vector loads beyond gout, out and the winner
// bytes; aligned_what: the family's sentence for the whole alignment rule.
static int kd_level_bwd_args_ok(const char *who, const float *gout, const float *out, const uint8_t *win, int64_t ldx, int64_t sel_stride, bool has_dx,
                                int64_t ldd, int dim, int Cin, bool more_aligned, const char *aligned_what, const void *workspace, size_t workspace_bytes,
                                size_t need)
{
    PAPC_REQUIRE(ldx >= Cin && (sel_stride == 0 || sel_stride >= dim) && (!has_dx || ldd >= Cin), PAPC_E_INVALID,
                 "%s: ldx=%lld < Cin, ldd=%lld < Cin or sel_stride=%lld (0 or >= dim)", who, (long long)ldx, (long long)ldd, (long long)sel_stride);
    PAPC_REQUIRE(Cin == 3 || (aligned16(gout) && aligned16(out) && (reinterpret_cast<uintptr_t>(win) & 7) == 0 && more_aligned), PAPC_E_INVALID, "%s: %s", who,
                 aligned_what);
    PAPC_REQUIRE(workspace_bytes >= need && aligned16(workspace), PAPC_E_INVALID, "%s: workspace %zu bytes < %zu (or not 16-byte aligned)", who, workspace_bytes,
                 need);
    return PAPC_OK;
}

}  // namespace papc
