// cloud_concat.hip -- the first seg_net layer of the PointNet part segmenters, for gfx950.
//
// Reference: PAPC/models/segment/pointnet/pointnet.py:105-107 and pointnet_base/pointnet_base.py:32-35:
//     x = concat([point_feat (Cp ch), tile(global_feat (Cg ch), N)]);  y = Conv1D(Cp + Cg, Cout, 1)(x)
// The tiled half is the same for every point of a cloud, so with W = [W_p | W_g] (W_p = W[:, :Cp]):
//     y[b, n, :] = W_p . x[b, n, :] + c[b, :]          c[b, :] = W_g . g[b, :] + bias
// and, with s[b] = sum_n dY[b, n, :] (the per-cloud column sums of dY):
//     dW_g = s^T . g    d bias = sum_b s[b]    dg = s . W_g    dX_p = dY . W_p    dW_p = dY^T . X_p
// No [B*N, Cp + Cg] tile is ever formed; the per-point GEMMs have K = Cp = 64.
//
//   forward   cc_cvec_kernel (c, one wave per output, a fixed DPP tree over Cg) and cc_fwd_kernel (128 x 128 tiles of y, plus the
//             per-tile column sums / sums of squares of y in papc_bn_finalize_f32's [n_tiles][2][Cout] layout).
//   backward  cc_bwd_kernel: ONE pass over (dz, y) in chunks of 128 rows of one cloud.  dY is formed on the fly from the layer's BN
//             constants (as every backward kernel of the stack does), a chunk writes its dX rows, its partial dW_p and its partial column
//             sums to slots of its own; cc_fold_kernel folds them in chunk order (fold.h); cc_tail_kernel forms dW_g, d bias and dg from s.
//             No float atomics: two runs are bit-identical.
// cloud_concat.h holds what this family shares with the K-looped one (cloud_concat_k.hip): the forward epilogue, dY, the fold of s, the
// argument checks.  cc_cvec_kernel and cc_tail_kernel are defined here and serve both families through cc_launch_cvec / cc_launch_tail.
// Products: v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation: the PAPC_GEMM_F32 arithmetic of papc_mlp_gemm_f32).  At
// K = 64 the layer is bound by the [M, Cout] traffic of y and dY, not by the matrix rate.  The small per-cloud products are fmaf chains
// in ascending index order.  Plain C++ loads and stores only.
#include "carve.h"
#include "cloud_concat.h"

namespace papc {

constexpr int CC_BN = 128;       // output columns per forward tile
constexpr int CC_CP = 64;        // the point-feature width the kernels are written for
constexpr int CC_OB = 64;        // output columns per backward column block
constexpr int CC_LDA = 68;       // LDS pitch (floats) of the float4-read tiles
constexpr int CC_LDX = 65;       // LDS pitch of the backward x tile (scalar reads)

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// c[b, o] = bias[o] + sum_k W[o, Cp + k] g[b, k]: workgroup (16 outputs, cloud b), wave = 4 outputs, lane = k (mod 64)
__global__ __launch_bounds__(CC_T) void cc_cvec_kernel(const float *__restrict__ g, const float *__restrict__ w, int64_t ldw, const float *__restrict__ bias,
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

// y tile [128 rows, 128 columns] = x . W_p^T + c[b(row)]; 4 waves of 64 x 64 (2 x 2 MFMA blocks); K = 64 staged whole in LDS; the epilogue
// (c[b(row)], the store, the tile's BatchNorm partials) is cloud_concat.h's
__global__ __launch_bounds__(CC_T) void cc_fwd_kernel(const float *__restrict__ x, int64_t ldx, const float *__restrict__ w, int64_t ldw,
                                                      const float *__restrict__ cvec, int M, int N, int Cout, float *__restrict__ y,
                                                      float *__restrict__ stats)
{
    __shared__ float xs[CC_BM * CC_LDA];
    __shared__ float ws[CC_BN * CC_LDA];
    __shared__ float red[2][2][CC_BN];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int n0 = blockIdx.x * CC_BN;
    const int m0 = blockIdx.y * CC_BM;
    for (int e = tid; e < CC_BM * 16; e += CC_T) {
        const int r = e >> 4, q = (e & 15) * 4;
        const int m = m0 + r;
        st4(&xs[r * CC_LDA + q], m < M ? ld4(x + (int64_t)m * ldx + q) : make_float4(0.f, 0.f, 0.f, 0.f));
        st4(&ws[r * CC_LDA + q], ld4(w + (int64_t)(n0 + r) * ldw + q));
    }
    __syncthreads();
    const int wm = wv & 1, wn = wv >> 1;
    floatx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // 32x32x2: lane supplies A[row l31][k] and B[k][col l31]; the two k of one instruction are kk + j (hi = 0) and kk + 4 + j (hi = 1)
#pragma unroll
    for (int kk = 0; kk < CC_CP; kk += 8) {
        float4 a[2], bq[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = ld4(&xs[(wm * 64 + i * 32 + l31) * CC_LDA + kk + 4 * hi]);
#pragma unroll
        for (int j = 0; j < 2; ++j) bq[j] = ld4(&ws[(wn * 64 + j * 32 + l31) * CC_LDA + kk + 4 * hi]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, bq[j].x, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, bq[j].y, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, bq[j].z, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, bq[j].w, acc[i][j], 0, 0, 0);
            }
    }
    cc_fwd_epilogue<2, 2, CC_BN>(acc, red, cvec, wm, wn, blockIdx.y, m0, n0, M, N, Cout, y, stats);
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// chunk (blockIdx.x) of cloud b (blockIdx.y): rows n0 .. n0 + 127 of the cloud (fewer in its last chunk).  Per column block of 64 outputs:
// dY block -> LDS; dX [128, 64] += dY_blk . W_p_blk (wave = 32 rows, 2 MFMA blocks, kept over the column blocks); partial dW_p [64, 64] =
// dY_blk^T . X (wave = one 32 x 32 block, K = the chunk's rows); partial column sums of dY.
__global__ __launch_bounds__(CC_T) void cc_bwd_kernel(const float *__restrict__ dz, const float *__restrict__ yv, const float *__restrict__ mean,
                                                      const float *__restrict__ invstd, const float *__restrict__ scale, const float *__restrict__ shift,
                                                      const float *__restrict__ c1, const float *__restrict__ c2, const float *__restrict__ x, int64_t ldx,
                                                      const float *__restrict__ w, int64_t ldw, int N, int Cout, float *dx, int64_t ldd, int accumulate,
                                                      float *__restrict__ part_w, float *__restrict__ part_s)
{
    __shared__ float xs[CC_BM * CC_LDX];
    __shared__ float gs[CC_BM * CC_LDA];
    __shared__ float wt[CC_CP * CC_LDA];       // W_p block transposed: wt[k][o]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int b = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
    const int n0 = ch * CC_BM;
    const int rows = min(CC_BM, N - n0);
    const int64_t mr0 = (int64_t)b * N + n0;
    const int64_t slot = (int64_t)b * nch + ch;
    for (int e = tid; e < CC_BM * 16; e += CC_T) {
        const int r = e >> 4, q = (e & 15) * 4;
        const float4 v = r < rows ? ld4(x + (mr0 + r) * ldx + q) : make_float4(0.f, 0.f, 0.f, 0.f);
        xs[r * CC_LDX + q] = v.x; xs[r * CC_LDX + q + 1] = v.y; xs[r * CC_LDX + q + 2] = v.z; xs[r * CC_LDX + q + 3] = v.w;
    }
    floatx16 dxa[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) dxa[j][r] = 0.f;
    for (int o0 = 0; o0 < Cout; o0 += CC_OB) {
        __syncthreads();                 // (the previous block's readers of gs / wt are done; the first time: xs is written)
        for (int e = tid; e < CC_BM * (CC_OB / 4); e += CC_T) {
            const int r = e >> 4, q = (e & 15) * 4, o = o0 + q;
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rows) {
                const float4 zz = ld4(dz + (mr0 + r) * Cout + o), yy = ld4(yv + (mr0 + r) * Cout + o);
                cc_dy4(d, zz, yy, ld4(scale + o), ld4(shift + o), ld4(mean + o), ld4(invstd + o), ld4(c1 + o), ld4(c2 + o));
            }
            st4(&gs[r * CC_LDA + q], d);
        }
        for (int e = tid; e < CC_OB * (CC_CP / 4); e += CC_T) {
            const int o = e >> 4, k = (e & 15) * 4;
            const float4 v = ld4(w + (int64_t)(o0 + o) * ldw + k);
            wt[k * CC_LDA + o] = v.x; wt[(k + 1) * CC_LDA + o] = v.y; wt[(k + 2) * CC_LDA + o] = v.z; wt[(k + 3) * CC_LDA + o] = v.w;
        }
        __syncthreads();
        // dX[m][k] += sum_o dY[m][o] W[o][k]:  A[m][o] = gs, B[o][k] = wt[k][o]
#pragma unroll
        for (int oo = 0; oo < CC_OB; oo += 8) {
            const float4 a = ld4(&gs[(wv * 32 + l31) * CC_LDA + oo + 4 * hi]);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float4 bq = ld4(&wt[(j * 32 + l31) * CC_LDA + oo + 4 * hi]);
                dxa[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bq.x, dxa[j], 0, 0, 0);
                dxa[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bq.y, dxa[j], 0, 0, 0);
                dxa[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bq.z, dxa[j], 0, 0, 0);
                dxa[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bq.w, dxa[j], 0, 0, 0);
            }
        }
        // partial dW_p[o][k] = sum_r dY[r][o] X[r][k]:  A[o][r] = gs[r][o], B[r][k] = xs[r][k]; wave: o block (wv & 1), k block (wv >> 1)
        const int ob = (wv & 1) * 32, kb = (wv >> 1) * 32;
        floatx16 dwa;
#pragma unroll
        for (int r = 0; r < 16; ++r) dwa[r] = 0.f;
#pragma unroll 8
        for (int r0 = 0; r0 < CC_BM; r0 += 2)
            dwa = __builtin_amdgcn_mfma_f32_32x32x2f32(gs[(r0 + hi) * CC_LDA + ob + l31], xs[(r0 + hi) * CC_LDX + kb + l31], dwa, 0, 0, 0);
        float *pw = part_w + (slot * Cout + o0 + ob) * CC_CP + kb + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) pw[(int64_t)((r & 3) + 8 * (r >> 2) + 4 * hi) * CC_CP] = dwa[r];
        // partial column sums: lane = column 16 wv + (lane & 15), rows 32 (lane >> 4) .. + 31, then the four row quarters in fixed order
        {
            const int cl = wv * 16 + (lane & 15), rq = (lane >> 4) * 32;
            float sacc = 0.f;
#pragma unroll 8
            for (int r = 0; r < 32; ++r) sacc += gs[(rq + r) * CC_LDA + cl];
            sacc += __shfl_xor(sacc, 16);
            sacc += __shfl_xor(sacc, 32);
            if (lane < 16) part_s[slot * Cout + o0 + cl] = sacc;
        }
    }
    if (dx) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (rr < rows) {
                    float *p = dx + (mr0 + rr) * ldd + j * 32 + l31;
                    *p = accumulate ? *p + dxa[j][r] : dxa[j][r];
                }
            }
    }
}

// dW_p[o][k] (into w's layout, ldw) = sum over the T = B * nch chunks; s[b][o] = sum over cloud b's nch chunks (fold.h: both in order from 0.f)
__global__ __launch_bounds__(CC_T) void cc_fold_kernel(const float *__restrict__ part_w, const float *__restrict__ part_s, int B, int nch, int Cout,
                                                       float *__restrict__ dw, int64_t ldw, float *__restrict__ s)
{
    const int64_t t = (int64_t)blockIdx.x * CC_T + threadIdx.x;
    const int64_t nw = (int64_t)Cout * CC_CP;
    if (t < nw) {
        dw[(t / CC_CP) * ldw + (t % CC_CP)] = fold_in_order<4, FOLD_FROM_ZERO, float>(part_w, nw, B * nch, t);
        return;
    }
    cc_fold_s(part_s, B, nch, Cout, t - nw, s);
}

// from s [B, Cout]: dW_g[o][k] = sum_b s[b][o] g[b][k] (into w's layout at column Cp + k), dg[b][k] = sum_o s[b][o] W[o][Cp + k],
// d bias[o] = sum_b s[b][o]
__global__ __launch_bounds__(CC_T) void cc_tail_kernel(const float *__restrict__ s, const float *__restrict__ g, const float *__restrict__ w, int64_t ldw,
                                                       int B, int Cp, int Cg, int Cout, float *__restrict__ dw, float *__restrict__ dbias,
                                                       float *__restrict__ dg)
{
    const int64_t t = (int64_t)blockIdx.x * CC_T + threadIdx.x;
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

void cc_launch_cvec(hipStream_t st, const float *g, const float *w, int64_t ldw, const float *bias, int B, int Cp, int Cg, int Cout, float *cvec)
{
    hipLaunchKernelGGL(cc_cvec_kernel, dim3((unsigned)(Cout / 16), (unsigned)B), dim3(CC_T), 0, st, g, w, ldw, bias, Cp, Cg, Cout, cvec);
}

void cc_launch_tail(hipStream_t st, const float *s, const float *g, const float *w, int64_t ldw, int B, int Cp, int Cg, int Cout, float *dw, float *dbias,
                    float *dg)
{
    const int64_t n_tail = (int64_t)Cout * Cg + (dg ? (int64_t)B * Cg : 0) + (dbias ? Cout : 0);
    hipLaunchKernelGGL(cc_tail_kernel, dim3((unsigned)cdiv(n_tail, CC_T)), dim3(CC_T), 0, st, s, g, w, ldw, B, Cp, Cg, Cout, dw, dbias, dg);
}

static int cc_shape_ok(const char *who, int B, int N, int Cp, int Cg, int Cout)
{
    PAPC_REQUIRE(Cp == CC_CP && Cg >= 64 && Cg <= 1024 && Cg % 64 == 0 && Cout == 512, PAPC_E_UNSUPPORTED,
                 "%s: Cp=%d Cg=%d Cout=%d (Cp = 64, Cg in 64..1024 and a multiple of 64, Cout = 512)", who, Cp, Cg, Cout);
    return cc_range_ok(who, B, N);
}

static int64_t cc_chunks(int N) { return cdiv(N, CC_BM); }

// workspace of the backward: [dW_p partials per chunk | column-sum partials per chunk | s]
struct CcBwdPtrs { float *part_w, *part_s, *s; };
static size_t cc_bwd_layout(int B, int N, int Cout, void *base, CcBwdPtrs &p)
{
    WsCarver c{static_cast<char *>(base), 0, 16};
    const size_t T = (size_t)B * (size_t)cc_chunks(N);
    p.part_w = c.take<float>(T * Cout * CC_CP); p.part_s = c.take<float>(T * Cout); p.s = c.take<float>((size_t)B * Cout);
    return c.off;
}

}  // namespace papc

using namespace papc;

extern "C" {

int papc_cloud_concat_conv_parts(int B, int N) { return cc_parts(B, N); }

int papc_cloud_concat_conv_f32(const float *x, int64_t ldx, const float *g, const float *w, const float *bias, int B, int N, int Cp, int Cg, int Cout,
                               float *y, float *cvec, float *stats_partial, papc_stream_t stream)
{
    const int err = cc_fwd_args_ok("papc_cloud_concat_conv_f32", cc_shape_ok, x, ldx, g, w, B, N, Cp, Cg, Cout, y, cvec);
    if (err != PAPC_OK) return err;
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    const int64_t ldw = (int64_t)Cp + Cg;
    const int M = B * N;
    cc_launch_cvec(st, g, w, ldw, bias, B, Cp, Cg, Cout, cvec);
    const int e = check_launch("papc_cloud_concat_conv_f32: c");
    if (e != PAPC_OK) return e;
    hipLaunchKernelGGL(cc_fwd_kernel, dim3((unsigned)(Cout / CC_BN), (unsigned)cdiv(M, CC_BM)), dim3(CC_T), 0, st, x, ldx, w, ldw, cvec, M, N, Cout, y,
                       stats_partial);
    return check_launch("papc_cloud_concat_conv_f32");
}

size_t papc_cloud_concat_conv_bwd_workspace(int B, int N, int Cp, int Cg, int Cout)
{
    if (B < 1 || N < 1 || Cp != CC_CP || Cout != 512 || Cg < 64 || Cg > 1024 || Cg % 64) return 0;
    CcBwdPtrs p;
    return cc_bwd_layout(B, N, Cout, nullptr, p);
}

int papc_cloud_concat_conv_bwd_f32(const float *dz, const float *y, const float *mean, const float *invstd, const float *scale, const float *shift,
                                   const float *c1, const float *c2, const float *x, int64_t ldx, const float *g, const float *w, int B, int N, int Cp,
                                   int Cg, int Cout, float *dx, int64_t ldd, int accumulate, float *dw, float *dbias, float *dg, float *s_out,
                                   void *workspace, size_t workspace_bytes, papc_stream_t stream)
{
    const int err = cc_bwd_args_ok("papc_cloud_concat_conv_bwd_f32", cc_shape_ok, dz, y, mean, invstd, scale, shift, c1, c2, x, ldx, g, w, B, N, Cp, Cg,
                                   Cout, dx, ldd, dw, workspace, true);
    if (err != PAPC_OK) return err;
    CcBwdPtrs p;
    const size_t need = cc_bwd_layout(B, N, Cout, workspace, p);
    PAPC_REQUIRE(workspace_bytes >= need, PAPC_E_INVALID, "papc_cloud_concat_conv_bwd_f32: workspace %zu bytes < %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    const int64_t ldw = (int64_t)Cp + Cg;
    const int nch = (int)cc_chunks(N);
    float *part_w = p.part_w, *part_s = p.part_s, *s = s_out ? s_out : p.s;
    hipLaunchKernelGGL(cc_bwd_kernel, dim3((unsigned)nch, (unsigned)B), dim3(CC_T), 0, st, dz, y, mean, invstd, scale, shift, c1, c2, x, ldx, w, ldw, N,
                       Cout, dx, ldd, accumulate, part_w, part_s);
    int e = check_launch("papc_cloud_concat_conv_bwd_f32");
    if (e != PAPC_OK) return e;
    const int64_t n_fold = (int64_t)Cout * CC_CP + (int64_t)B * Cout;
    hipLaunchKernelGGL(cc_fold_kernel, dim3((unsigned)cdiv(n_fold, CC_T)), dim3(CC_T), 0, st, part_w, part_s, B, nch, Cout, dw, ldw, s);
    e = check_launch("papc_cloud_concat_conv_bwd_f32: fold");
    if (e != PAPC_OK) return e;
    cc_launch_tail(st, s, g, w, ldw, B, Cp, Cg, Cout, dw, dbias, dg);
    return check_launch("papc_cloud_concat_conv_bwd_f32: tail");
}

}  // extern "C"
