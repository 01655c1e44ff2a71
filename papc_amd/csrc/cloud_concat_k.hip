// cloud_concat_k.hip -- the wide concat convs of the VFE models, for gfx950: a 1x1 conv over concat([x (Cp ch), tile(g (Cg ch), N)]), K-looped.
//
// Reference: PAPC/models/classify/vfe/vfe.py:79-83 (vfe.pointnet_2.mlp_1.0: Cp = 256, Cg = 256, Cout = 64) and
// PAPC/models/segment/vfe/vfe.py:33-36 (seg_net[0]: Cp = 256, Cg = 256 + max_points, Cout = 512).  As in cloud_concat.hip the tiled half is the
// same for every point of a cloud, so with W = [W_p | W_g] (W_p = W[:, :Cp]):
//     y[b, n, :] = W_p . x[b, n, :] + c[b, :]          c[b, :] = W_g . g[b, :] + bias
// and, with s[b] = sum_n dY[b, n, :]:
//     dX_p = dY . W_p    dW_p = dY^T . X_p    dW_g = s^T . g    d bias = sum_b s[b]    dg = s . W_g
// No [B*N, Cp + Cg] tile is ever formed.  cloud_concat.hip stages its whole K = 64 and runs exact fp32 products because that layer is bound
// by the traffic of y; at K = 256 the per-point products sit on the matrix pipe, so they run on v_mfma_f32_32x32x16_bf16 through bf16x3.h.
//
//   forward   cck_cvec_kernel (c, one wave per output, a fixed DPP tree over Cg) and cck_fwd_kernel<BN>: tiles of 128 rows x BN columns of y
//             (BN = 128 where Cout is a multiple of 128, else 64: no tile runs on padding columns), a K loop over Cp in stages of 32 through
//             LDS with the next stage's global loads in flight.  Lane (r = lane & 31, h = lane >> 5) holds A[row r][k = 8h + j] and
//             B[k = 8h + j][col r]; accumulator register i is row (i & 3) + 8 (i >> 2) + 4h of column r (the layout at the top of voxconv.hip).
//             A tile may straddle clouds: the epilogue picks c[b(m)] per row.  Rows past M are neither stored nor counted in the per-tile
//             column sums / sums of squares (papc_bn_finalize_f32's [tiles][2][Cout] layout).
//   backward  dX_p and dW_p are the stack's own products: papc_mlp_bwd_dx_f32 against W_p^T (cck_wt_kernel writes it once per call) and
//             papc_mlp_bwd_dw_f32 over at most CK_MAX_RANGES row ranges, folded by papc_reduce_partials_strided_f32 into w's layout -- dY formed
//             on the fly from (dz, y) and the layer's BN constants in both.  New here: cck_colsum_kernel (per-cloud column sums of dY, per
//             128-row segment of a cloud), cck_fold_kernel (segments in order, fold.h) and cck_tail_kernel (dW_g, d bias, dg from s).
// No float atomics, every cross-workgroup sum a fixed-order fold: two runs are bit-identical.  The small per-cloud products are fmaf chains in
// ascending index order.  Plain C++ loads and stores; every k loop is straight-line (operands always loaded from addresses that exist, then
// selected) and cck_drain holds the accumulators over the last MFMA's passes in front of the epilogue.
#include "bf16x3.h"
#include "fold.h"

namespace papc {

constexpr int CK_T = 256;            // threads of every kernel here (4 waves)
constexpr int CK_BM = 128;           // rows per forward tile / per column-sum segment
constexpr int CK_KS = 32;            // floats of K per forward stage
constexpr int CK_LD = 36;            // LDS pitch (floats) of a stage's rows: 16-byte aligned, 4 banks off per row
constexpr int CK_MAX_RANGES = 64;    // row ranges of the dW_p partials (each a [Cout, Cp] block: at most 32 MB at Cp = 256, Cout = 512)

__device__ __forceinline__ float4 ck_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void ck_st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ void ck_ld8(const float *p, float (&v)[8])
{
    const float4 a = ck_ld4(p), b = ck_ld4(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void cck_drain(floatx16 &acc) { asm volatile("s_nop 15" : "+a"(acc)); }

// dy = scale (p - c1 - xhat c2), p = dz where scale y + shift > 0 (mlp_loaders.h: dy_elem; cloud_concat.hip forms it the same way)
__device__ __forceinline__ float ck_dy(float zz, float yy, float sc, float sh, float mu, float is, float k1, float k2)
{
    return sc * ((((fmaf(sc, yy, sh) > 0.f) ? zz : 0.f) - k1) - (yy - mu) * is * k2);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// c[b, o] = bias[o] + sum_k W[o, Cp + k] g[b, k]: workgroup (16 outputs, cloud b), wave = 4 outputs, lane = k (mod 64)
__global__ __launch_bounds__(CK_T) void cck_cvec_kernel(const float *__restrict__ g, const float *__restrict__ w, int64_t ldw, const float *__restrict__ bias,
                                                        int Cp, int Cg, int Cout, float *__restrict__ cvec)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float *gb = g + (int64_t)b * Cg;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int o = blockIdx.x * 16 + wv * 4 + q;
        const float *wr = w + (int64_t)o * ldw + Cp;
        float a = 0.f;
        for (int k = lane; k < Cg; k += 64) a = fmaf(wr[k], gb[k], a);
        a = wave_sum_f32_to_lane63(a);
        if (lane == 63) cvec[(int64_t)b * Cout + o] = bias ? a + bias[o] : a;
    }
}

// y tile [128 rows, BN columns] = x . W_p^T + c[b(row)].  BN = 128: 2 x 2 waves of 64 x 64 (2 x 2 MFMA blocks); BN = 64: 4 x 1 waves of 32 x 64.
// Workgroup blockIdx.x = row tile * (Cout / BN) + column block (the column blocks of a row tile run next to each other: x is read from HBM once).
template <int BN>
__global__ __launch_bounds__(CK_T) void cck_fwd_kernel(const float *__restrict__ x, int64_t ldx, const float *__restrict__ w, int64_t ldw,
                                                       const float *__restrict__ cvec, int M, int N, int Cp, int Cout, float *__restrict__ y,
                                                       float *__restrict__ stats)
{
    constexpr int IB = BN == 128 ? 2 : 1;        // 32-row blocks of a wave
    constexpr int WMW = BN == 128 ? 2 : 4;       // waves along the rows
    constexpr int NWR = BN / 32;                 // float4 of the W stage per thread
    __shared__ float xs[CK_BM * CK_LD];
    __shared__ float ws[BN * CK_LD];
    __shared__ float red[WMW][2][BN];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int ncb = Cout / BN;
    const int tile = blockIdx.x / ncb, n0 = (blockIdx.x - tile * ncb) * BN;
    const int m0 = tile * CK_BM;
    const int wm = wv % WMW, wn = wv / WMW;
    const int sr = tid >> 3, sq = (tid & 7) * 4;         // this thread's row (+ 32 i) and k offset within a stage
    float4 xr[4], wr[NWR];
    const float *xp[4];
    bool xlive[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + sr + 32 * i;
        xlive[i] = m < M;
        xp[i] = x + (int64_t)(xlive[i] ? m : M - 1) * ldx + sq;
    }
    const float *wp = w + (int64_t)(n0 + sr) * ldw + sq;
#pragma unroll
    for (int i = 0; i < 4; ++i) xr[i] = ck_ld4(xp[i]);
#pragma unroll
    for (int i = 0; i < NWR; ++i) wr[i] = ck_ld4(wp + (int64_t)(32 * i) * ldw);
    floatx16 acc[IB][2];
#pragma unroll
    for (int i = 0; i < IB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int k0 = 0; k0 < Cp; k0 += CK_KS) {
        __syncthreads();                             // the previous stage's readers are done
#pragma unroll
        for (int i = 0; i < 4; ++i) ck_st4(&xs[(sr + 32 * i) * CK_LD + sq], xlive[i] ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f));
#pragma unroll
        for (int i = 0; i < NWR; ++i) ck_st4(&ws[(sr + 32 * i) * CK_LD + sq], wr[i]);
        __syncthreads();
        const int kn = min(k0 + CK_KS, Cp - CK_KS);  // the next stage in flight over this one's products (the last stage re-reads itself)
#pragma unroll
        for (int i = 0; i < 4; ++i) xr[i] = ck_ld4(xp[i] + kn);
#pragma unroll
        for (int i = 0; i < NWR; ++i) wr[i] = ck_ld4(wp + (int64_t)(32 * i) * ldw + kn);
#pragma unroll
        for (int kk = 0; kk < CK_KS; kk += 16) {
            bf16x8 ap[IB][3], bp[2][3];
#pragma unroll
            for (int i = 0; i < IB; ++i) {
                float v[8];
                ck_ld8(&xs[((wm * IB + i) * 32 + l31) * CK_LD + kk + 8 * hi], v);
                split8(v, ap[i]);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float v[8];
                ck_ld8(&ws[(wn * 64 + j * 32 + l31) * CK_LD + kk + 8 * hi], v);
                split8(v, bp[j]);
            }
#pragma unroll
            for (int i = 0; i < IB; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma_bf16x3(ap[i], bp[j], acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < IB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) cck_drain(acc[i][j]);
    // epilogue: register r is row (r & 3) + 8 (r >> 2) + 4 hi of column l31.  Rows past M are neither stored nor counted.
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
    for (int j = 0; j < 2; ++j) {       // the two row halves of a lane pair, then the tile's waves along the rows in order
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

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// wt[k][o] = w[o][k], k < Cp: the operand papc_mlp_bwd_dx_f32 takes
__global__ __launch_bounds__(CK_T) void cck_wt_kernel(const float *__restrict__ w, int64_t ldw, int Cp, int Cout, float *__restrict__ wt)
{
    const int t = blockIdx.x * CK_T + threadIdx.x;
    if (t >= Cp * Cout) return;
    const int k = t / Cout, o = t - k * Cout;
    wt[t] = w[(int64_t)o * ldw + k];
}

// partial column sums of dY over segment blockIdx.x (128 rows) of cloud blockIdx.y: thread = (four columns, row group); a row group walks its
// rows in ascending order, the groups are added in order
__global__ __launch_bounds__(CK_T) void cck_colsum_kernel(const float *__restrict__ dz, const float *__restrict__ yv, const float *__restrict__ mean,
                                                          const float *__restrict__ invstd, const float *__restrict__ scale, const float *__restrict__ shift,
                                                          const float *__restrict__ c1, const float *__restrict__ c2, int N, int Cout,
                                                          float *__restrict__ part_s)
{
    __shared__ float4 red[CK_T];
    const int tid = threadIdx.x;
    const int ncq = Cout / 4, nrg = CK_T / ncq;
    const int cq = tid % ncq, rg = tid / ncq;
    const int b = blockIdx.y, n0 = blockIdx.x * CK_BM;
    const int rows = min(CK_BM, N - n0);
    const int64_t mr0 = (int64_t)b * N + n0;
    const int o = cq * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rg < nrg) {
        const float4 sc = ck_ld4(scale + o), sh = ck_ld4(shift + o), mu = ck_ld4(mean + o), is = ck_ld4(invstd + o), k1 = ck_ld4(c1 + o), k2 = ck_ld4(c2 + o);
        for (int r = rg; r < rows; r += nrg) {
            const float4 zz = ck_ld4(dz + (mr0 + r) * Cout + o), yy = ck_ld4(yv + (mr0 + r) * Cout + o);
            a.x += ck_dy(zz.x, yy.x, sc.x, sh.x, mu.x, is.x, k1.x, k2.x);
            a.y += ck_dy(zz.y, yy.y, sc.y, sh.y, mu.y, is.y, k1.y, k2.y);
            a.z += ck_dy(zz.z, yy.z, sc.z, sh.z, mu.z, is.z, k1.z, k2.z);
            a.w += ck_dy(zz.w, yy.w, sc.w, sh.w, mu.w, is.w, k1.w, k2.w);
        }
    }
    red[tid] = a;
    __syncthreads();
    if (rg == 0) {
        for (int t = 1; t < nrg; ++t) a = fold_add(a, red[t * ncq + cq]);
        ck_st4(part_s + ((int64_t)b * gridDim.x + blockIdx.x) * Cout + o, a);
    }
}

// s[b][o] = sum over cloud b's nseg segments, in order from 0.f (fold.h)
__global__ __launch_bounds__(CK_T) void cck_fold_kernel(const float *__restrict__ part_s, int B, int nseg, int Cout, float *__restrict__ s)
{
    const int64_t u = (int64_t)blockIdx.x * CK_T + threadIdx.x;
    if (u >= (int64_t)B * Cout) return;
    const int64_t b = u / Cout, o = u - b * Cout;
    s[u] = fold_in_order<1, FOLD_FROM_ZERO, float>(part_s, Cout, nseg, b * nseg * Cout + o);
}

// from s [B, Cout]: dW_g[o][k] = sum_b s[b][o] g[b][k] (into w's layout at column Cp + k), dg[b][k] = sum_o s[b][o] W[o][Cp + k],
// d bias[o] = sum_b s[b][o]
__global__ __launch_bounds__(CK_T) void cck_tail_kernel(const float *__restrict__ s, const float *__restrict__ g, const float *__restrict__ w, int64_t ldw,
                                                        int B, int Cp, int Cg, int Cout, float *__restrict__ dw, float *__restrict__ dbias,
                                                        float *__restrict__ dg)
{
    const int64_t t = (int64_t)blockIdx.x * CK_T + threadIdx.x;
    const int64_t n1 = (int64_t)Cout * Cg, n2 = n1 + (dg ? (int64_t)B * Cg : 0), n3 = n2 + (dbias ? Cout : 0);
    if (t < n1) {
        const int64_t o = t / Cg, k = t - o * Cg;
        float a = 0.f;
        for (int b = 0; b < B; ++b) a = fmaf(s[(int64_t)b * Cout + o], g[(int64_t)b * Cg + k], a);
        dw[o * ldw + Cp + k] = a;
    } else if (t < n2) {
        const int64_t u = t - n1, b = u / Cg, k = u - b * Cg;
        const float *sb = s + b * Cout;
        const float *wk = w + Cp + k;
        float a = 0.f;
#pragma unroll 8
        for (int o = 0; o < Cout; ++o) a = fmaf(sb[o], wk[(int64_t)o * ldw], a);
        dg[u] = a;
    } else if (t < n3) {
        const int64_t o = t - n2;
        float a = 0.f;
        for (int b = 0; b < B; ++b) a += s[(int64_t)b * Cout + o];
        dbias[o] = a;
    }
}

// dx[m][k] (+)= t[m][k]: the dense dX of papc_mlp_bwd_dx_f32 into a strided or accumulating destination
__global__ __launch_bounds__(CK_T) void cck_rows_out_kernel(const float *__restrict__ t, int64_t M, int Cp, float *__restrict__ dx, int64_t ldd, int accumulate)
{
    const int64_t e = (int64_t)blockIdx.x * CK_T + threadIdx.x;
    if (e >= M * Cp) return;
    const int64_t m = e / Cp, k = e - m * Cp;
    float *p = dx + m * ldd + k;
    *p = accumulate ? *p + t[e] : t[e];
}

static bool cck_widths_ok(int Cp, int Cg, int Cout)
{
    return Cp >= 64 && Cp <= 256 && Cp % 64 == 0 && Cout >= 64 && Cout <= 512 && Cout % 64 == 0 && Cg >= 64 && Cg <= 2304 && Cg % 64 == 0;
}

static int cck_shape_ok(const char *who, int B, int N, int Cp, int Cg, int Cout)
{
    PAPC_REQUIRE(cck_widths_ok(Cp, Cg, Cout), PAPC_E_UNSUPPORTED,
                 "%s: Cp=%d Cg=%d Cout=%d (multiples of 64: Cp in 64..256, Cg in 64..2304, Cout in 64..512)", who, Cp, Cg, Cout);
    PAPC_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && (int64_t)B * N <= ((int64_t)1 << 30), PAPC_E_INVALID, "%s: B=%d N=%d", who, B, N);
    return PAPC_OK;
}

// rows per dW_p range: at most CK_MAX_RANGES ranges, whole multiples of 64 rows, at least 256
static int64_t cck_rows_per_range(int64_t M) { return std::max<int64_t>(256, cdiv(cdiv(M, CK_MAX_RANGES), 64) * 64); }

struct CckWs { int64_t wt, part, part_ld, ranges, rpr, part_s, s, dxt, total; };   // offsets and sizes in floats

static CckWs cck_ws(int B, int N, int Cp, int Cout)
{
    CckWs l;
    const int64_t M = (int64_t)B * N;
    l.rpr = cck_rows_per_range(M);
    l.ranges = cdiv(M, l.rpr);
    l.part_ld = (int64_t)Cout * Cp + Cout;
    l.wt = 0;
    l.part = l.wt + (int64_t)Cp * Cout;
    l.part_s = l.part + l.ranges * l.part_ld;
    l.s = l.part_s + (int64_t)B * cdiv(N, CK_BM) * Cout;
    l.dxt = l.s + (int64_t)B * Cout;
    l.total = l.dxt + M * Cp;
    return l;
}

}  // namespace papc

using namespace papc;

extern "C" {

int papc_cloud_concat_k_ok(int Cp, int Cg, int Cout) { return cck_widths_ok(Cp, Cg, Cout) ? 1 : 0; }

int papc_cloud_concat_k_parts(int B, int N)
{
    if (B < 1 || N < 1) return 0;
    return (int)cdiv((int64_t)B * N, CK_BM);
}

int papc_cloud_concat_k_f32(const float *x, int64_t ldx, const float *g, const float *w, const float *bias, int B, int N, int Cp, int Cg, int Cout,
                            float *y, float *cvec, float *stats_partial, papc_stream_t stream)
{
    PAPC_REQUIRE(x && g && w && y && cvec, PAPC_E_INVALID, "papc_cloud_concat_k_f32: null pointer");
    const int err = cck_shape_ok("papc_cloud_concat_k_f32", B, N, Cp, Cg, Cout);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(ldx >= Cp && ldx % 4 == 0 && aligned16(x) && aligned16(w), PAPC_E_INVALID,
                 "papc_cloud_concat_k_f32: x and w must be 16-byte aligned, ldx=%lld a multiple of 4 >= Cp", (long long)ldx);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    const int64_t ldw = (int64_t)Cp + Cg;
    const int M = B * N;
    hipLaunchKernelGGL(cck_cvec_kernel, dim3((unsigned)(Cout / 16), (unsigned)B), dim3(CK_T), 0, st, g, w, ldw, bias, Cp, Cg, Cout, cvec);
    const int e = check_launch("papc_cloud_concat_k_f32: c");
    if (e != PAPC_OK) return e;
    const int64_t tiles = cdiv(M, CK_BM);
    if (Cout % 128 == 0)
        hipLaunchKernelGGL(cck_fwd_kernel<128>, dim3((unsigned)(tiles * (Cout / 128))), dim3(CK_T), 0, st, x, ldx, w, ldw, cvec, M, N, Cp, Cout, y,
                           stats_partial);
    else
        hipLaunchKernelGGL(cck_fwd_kernel<64>, dim3((unsigned)(tiles * (Cout / 64))), dim3(CK_T), 0, st, x, ldx, w, ldw, cvec, M, N, Cp, Cout, y,
                           stats_partial);
    return check_launch("papc_cloud_concat_k_f32");
}

size_t papc_cloud_concat_k_bwd_workspace(int B, int N, int Cp, int Cg, int Cout)
{
    if (B < 1 || N < 1 || B > 65535 || (int64_t)B * N > ((int64_t)1 << 30) || !cck_widths_ok(Cp, Cg, Cout)) return 0;
    return (size_t)cck_ws(B, N, Cp, Cout).total * sizeof(float);
}

int papc_cloud_concat_k_bwd_f32(const float *dz, const float *y, const float *mean, const float *invstd, const float *scale, const float *shift,
                                const float *c1, const float *c2, const float *x, int64_t ldx, const float *g, const float *w, int B, int N, int Cp,
                                int Cg, int Cout, float *dx, int64_t ldd, int accumulate, float *dw, float *dbias, float *dg, float *s_out,
                                void *workspace, size_t workspace_bytes, papc_stream_t stream)
{
    PAPC_REQUIRE(dz && y && mean && invstd && scale && shift && c1 && c2 && x && g && w && dw && workspace, PAPC_E_INVALID,
                 "papc_cloud_concat_k_bwd_f32: null pointer");
    const int err = cck_shape_ok("papc_cloud_concat_k_bwd_f32", B, N, Cp, Cg, Cout);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(ldx >= Cp && ldx % 4 == 0 && aligned16(x) && aligned16(w) && aligned16(dz) && aligned16(y) && aligned16(mean) && aligned16(invstd)
                 && aligned16(scale) && aligned16(shift) && aligned16(c1) && aligned16(c2) && aligned16(workspace) && (!dx || ldd >= Cp), PAPC_E_INVALID,
                 "papc_cloud_concat_k_bwd_f32: operands must be 16-byte aligned, ldx=%lld a multiple of 4 >= Cp, ldd=%lld >= Cp",
                 (long long)ldx, (long long)ldd);
    const size_t need = papc_cloud_concat_k_bwd_workspace(B, N, Cp, Cg, Cout);
    PAPC_REQUIRE(workspace_bytes >= need, PAPC_E_INVALID, "papc_cloud_concat_k_bwd_f32: workspace %zu bytes < %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const int64_t ldw = (int64_t)Cp + Cg;
    const int64_t M = (int64_t)B * N;
    const int nseg = (int)cdiv(N, CK_BM);
    const CckWs l = cck_ws(B, N, Cp, Cout);
    float *base = static_cast<float *>(workspace);
    float *wt = base + l.wt, *part = base + l.part, *part_s = base + l.part_s, *dxt = base + l.dxt;
    float *s = s_out ? s_out : base + l.s;
    int e;
    {
        ProfScope prof(PAPC_K_MISC, st);
        hipLaunchKernelGGL(cck_colsum_kernel, dim3((unsigned)nseg, (unsigned)B), dim3(CK_T), 0, st, dz, y, mean, invstd, scale, shift, c1, c2, N, Cout,
                           part_s);
        e = check_launch("papc_cloud_concat_k_bwd_f32: column sums");
        if (e != PAPC_OK) return e;
        hipLaunchKernelGGL(cck_fold_kernel, dim3((unsigned)cdiv((int64_t)B * Cout, CK_T)), dim3(CK_T), 0, st, part_s, B, nseg, Cout, s);
        e = check_launch("papc_cloud_concat_k_bwd_f32: fold");
        if (e != PAPC_OK) return e;
        if (dx) {
            hipLaunchKernelGGL(cck_wt_kernel, dim3((unsigned)cdiv((int64_t)Cp * Cout, CK_T)), dim3(CK_T), 0, st, w, ldw, Cp, Cout, wt);
            e = check_launch("papc_cloud_concat_k_bwd_f32: W_p^T");
            if (e != PAPC_OK) return e;
        }
    }
    papc_bwd_dy dy;
    memset(&dy, 0, sizeof(dy));
    dy.dz_mode = PAPC_DZ_DENSE; dy.dz = dz; dy.K = 1; dy.y = y;
    dy.mean = mean; dy.invstd = invstd; dy.scale = scale; dy.shift = shift; dy.c1 = c1; dy.c2 = c2;
    if (dx) {
        const bool direct = !accumulate && ldd == Cp;
        e = papc_mlp_bwd_dx_f32(&dy, wt, M, Cp, Cout, direct ? dx : dxt, nullptr, nullptr, stream);
        if (e != PAPC_OK) return e;
        if (!direct) {
            ProfScope prof(PAPC_K_MISC, st);
            hipLaunchKernelGGL(cck_rows_out_kernel, dim3((unsigned)cdiv(M * Cp, CK_T)), dim3(CK_T), 0, st, dxt, M, Cp, dx, ldd, accumulate);
            e = check_launch("papc_cloud_concat_k_bwd_f32: dX rows");
            if (e != PAPC_OK) return e;
        }
    }
    e = papc_mlp_bwd_dw_f32(&dy, PAPC_A_PLAIN, x, ldx, nullptr, nullptr, nullptr, M, Cp, Cout, (int)l.rpr, part, part + (int64_t)Cout * Cp, l.part_ld, stream);
    if (e != PAPC_OK) return e;
    e = papc_reduce_partials_strided_f32(part, (int)l.ranges, l.part_ld, Cout, Cp, dw, ldw, 0, stream);
    if (e != PAPC_OK) return e;
    ProfScope prof(PAPC_K_MISC, st);
    const int64_t n_tail = (int64_t)Cout * Cg + (dg ? (int64_t)B * Cg : 0) + (dbias ? Cout : 0);
    hipLaunchKernelGGL(cck_tail_kernel, dim3((unsigned)cdiv(n_tail, CK_T)), dim3(CK_T), 0, st, s, g, w, ldw, B, Cp, Cg, Cout, dw, dbias, dg);
    return check_launch("papc_cloud_concat_k_bwd_f32: tail");
}

}  // extern "C"
