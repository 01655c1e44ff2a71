// cloud_concat.h -- what the two concat-conv families share: cloud_concat.hip (Cp = 64 staged whole, exact fp32 products, a one-pass backward)
// and cloud_concat_k.hip (K-looped over Cp on bf16x3, dX_p / dW_p through the stack's own products).
//
// Both compute the 1x1 conv over concat([x (Cp ch), tile(g (Cg ch), N)]) with W = [W_p | W_g] as
//     y[b, n, :] = W_p . x[b, n, :] + c[b, :]          c[b, :] = W_g . g[b, :] + bias
// and, with s[b] = sum_n dY[b, n, :]:
//     dW_g = s^T . g    d bias = sum_b s[b]    dg = s . W_g
// Here: the forward tile epilogue (add c[b(row)], store, the per-tile BatchNorm partials), dY of four columns, the in-order fold of s, the host
// checks of the entry points' arguments, and the launchers of the two kernels that are the same in both families -- c (cc_cvec_kernel) and
// the tail that forms dW_g, d bias and dg from s (cc_tail_kernel); cloud_concat.hip defines them, each .hip being its own translation unit of
// one library.  The GEMM bodies and the backward strategies are each family's own.
#pragma once
#include "fold.h"
#include "mlp_loaders.h"

namespace papc {

constexpr int CC_T = 256;        // threads of every kernel of both families (4 waves)
constexpr int CC_BM = 128;       // rows per forward tile (cc_parts counts them) and per backward chunk / column-sum segment

__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }

// d = dY of four columns: dy = scale (p - c1 - xhat c2), p = dz where scale y + shift > 0
__device__ __forceinline__ void cc_dy4(float4 &d, float4 zz, float4 yy, float4 sc, float4 sh, float4 mu, float4 is, float4 k1, float4 k2)
{
    d.x = dy_elem(zz.x, yy.x, sc.x, sh.x, mu.x, is.x, k1.x, k2.x);
    d.y = dy_elem(zz.y, yy.y, sc.y, sh.y, mu.y, is.y, k1.y, k2.y);
    d.z = dy_elem(zz.z, yy.z, sc.z, sh.z, mu.z, is.z, k1.z, k2.z);
    d.w = dy_elem(zz.w, yy.w, sc.w, sh.w, mu.w, is.w, k1.w, k2.w);
}

// s[u], u = b Cout + o: the sum over cloud b's nseg partial column sums part_s[b][seg][o], in order from 0.f (fold.h)
__device__ __forceinline__ void cc_fold_s(const float *__restrict__ part_s, int B, int nseg, int Cout, int64_t u, float *__restrict__ s)
{
    if (u >= (int64_t)B * Cout) return;
    const int64_t b = u / Cout, o = u - b * Cout;
    s[u] = fold_in_order<1, FOLD_FROM_ZERO, float>(part_s, Cout, nseg, b * nseg * Cout + o);
}

// The epilogue of a forward tile [128 rows at m0, BN columns at n0] held by 4 waves, WMW of them along the rows (the calling wave is the
// wm-th along the rows, the wn-th along the columns), a wave IB x 2 MFMA blocks of 32 x 32: register r of acc[i][j] is row
// (wm IB + i) 32 + (r & 3) + 8 (r >> 2) + 4 hi of column wn 64 + j 32 + l31.  y = acc + c[b(row)] is stored -- a tile may straddle clouds -- and, where stats is given, the tile's column sums and sums
// of squares go to stats[tile][2][Cout] (papc_bn_finalize_f32's layout): a lane's rows in order, the two row halves of a lane pair, then the
// waves along the rows in order.  Rows past M are neither stored nor counted.  Every thread of the workgroup calls.
template <int IB, int WMW, int BN>
__device__ __forceinline__ void cc_fwd_epilogue(const floatx16 (&acc)[IB][2], float (&red)[WMW][2][BN], const float *cvec, int wm, int wn, int tile,
                                                int m0, int n0, int M, int N, int Cout, float *y, float *stats)
{
    const int tid = threadIdx.x, l31 = tid & 31, hi = (tid >> 5) & 1;
    float s1[2] = {0.f, 0.f}, s2[2] = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < IB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + (wm * IB + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (m < M) {
                const float *cb = cvec + (int64_t)(m / N) * Cout;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int col = n0 + wn * 64 + j * 32 + l31;
                    const float v = acc[i][j][r] + cb[col];
                    y[(int64_t)m * Cout + col] = v;
                    s1[j] += v;
                    s2[j] = fmaf(v, v, s2[j]);
                }
            }
        }
    if (!stats) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        s1[j] += __shfl_xor(s1[j], 32);
        s2[j] += __shfl_xor(s2[j], 32);
    }
    if (hi == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            red[wm][0][wn * 64 + j * 32 + l31] = s1[j];
            red[wm][1][wn * 64 + j * 32 + l31] = s2[j];
        }
    }
    __syncthreads();
    if (tid < 2 * BN) {
        const int q = tid / BN, cl = tid - q * BN;
        float a = red[0][q][cl];
#pragma unroll
        for (int t = 1; t < WMW; ++t) a += red[t][q][cl];
        stats[(int64_t)tile * 2 * Cout + (int64_t)q * Cout + n0 + cl] = a;
    }
}

// ---- the kernels both families launch (defined in cloud_concat.hip; no ProfScope of their own: the caller's covers them) -------------------
// c[b, o] = bias[o] + sum_k W[o, Cp + k] g[b, k]
void cc_launch_cvec(hipStream_t st, const float *g, const float *w, int64_t ldw, const float *bias, int B, int Cp, int Cg, int Cout, float *cvec);
// from s [B, Cout]: dW_g into w's layout at column Cp, dg and d bias (each may be NULL)
void cc_launch_tail(hipStream_t st, const float *s, const float *g, const float *w, int64_t ldw, int B, int Cp, int Cg, int Cout, float *dw, float *dbias,
                    float *dg);

// ---- the entry points' checks -------------------------------------------------------------------------------------------------------------
// a family's own: its widths (PAPC_E_UNSUPPORTED, its message), then cc_range_ok
typedef int (*cc_shape_fn)(const char *who, int B, int N, int Cp, int Cg, int Cout);

static inline int cc_parts(int B, int N)
{
    if (B < 1 || N < 1) return 0;
    return (int)cdiv((int64_t)B * N, CC_BM);
}

static inline int cc_range_ok(const char *who, int B, int N)
{
    PAPC_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && (int64_t)B * N <= ((int64_t)1 << 30), PAPC_E_INVALID, "%s: B=%d N=%d", who, B, N);
    return PAPC_OK;
}

static inline int cc_fwd_args_ok(const char *who, cc_shape_fn shape_ok, const float *x, int64_t ldx, const float *g, const float *w, int B, int N, int Cp,
                                 int Cg, int Cout, const float *y, const float *cvec)
{
    PAPC_REQUIRE(x && g && w && y && cvec, PAPC_E_INVALID, "%s: null pointer", who);
    const int err = shape_ok(who, B, N, Cp, Cg, Cout);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(ldx >= Cp && ldx % 4 == 0 && aligned16(x) && aligned16(w), PAPC_E_INVALID,
                 "%s: x and w must be 16-byte aligned, ldx=%lld a multiple of 4 >= Cp", who, (long long)ldx);
    return PAPC_OK;
}

// (ws_aligned: the K-looped family stores float4 into its workspace)
static inline int cc_bwd_args_ok(const char *who, cc_shape_fn shape_ok, const float *dz, const float *y, const float *mean, const float *invstd,
                                 const float *scale, const float *shift, const float *c1, const float *c2, const float *x, int64_t ldx, const float *g,
                                 const float *w, int B, int N, int Cp, int Cg, int Cout, const float *dx, int64_t ldd, const float *dw,
                                 const void *workspace, bool ws_aligned)
{
    PAPC_REQUIRE(dz && y && mean && invstd && scale && shift && c1 && c2 && x && g && w && dw && workspace, PAPC_E_INVALID, "%s: null pointer", who);
    const int err = shape_ok(who, B, N, Cp, Cg, Cout);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(ldx >= Cp && ldx % 4 == 0 && aligned16(x) && aligned16(w) && aligned16(dz) && aligned16(y) && aligned16(mean) && aligned16(invstd)
                 && aligned16(scale) && aligned16(shift) && aligned16(c1) && aligned16(c2) && ws_aligned && (!dx || ldd >= Cp), PAPC_E_INVALID,
                 "%s: operands must be 16-byte aligned, ldx=%lld a multiple of 4 >= Cp, ldd=%lld >= Cp", who, (long long)ldx, (long long)ldd);
    return PAPC_OK;
}

}  // namespace papc
