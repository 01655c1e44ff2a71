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
//   forward   cc_cvec_kernel (c; cloud_concat.hip's, through cc_launch_cvec) and cck_fwd_kernel<BN>: tiles of 128 rows x BN columns of y
//             (BN = 128 where Cout is a multiple of 128, else 64: no tile runs on padding columns), a K loop over Cp in stages of 32 through
//             LDS with the next stage's global loads in flight.  Lane (r = lane & 31, h = lane >> 5) holds A[row r][k = 8h + j] and
//             B[k = 8h + j][col r]; accumulator register i is row (i & 3) + 8 (i >> 2) + 4h of column r (the layout at the top of voxconv.hip).
//             The epilogue is cloud_concat.h's cc_fwd_epilogue, shared with cloud_concat.hip.
//   backward  dX_p and dW_p are the stack's own products: papc_mlp_bwd_dx_f32 against W_p^T (cck_wt_kernel writes it once per call) and
//             papc_mlp_bwd_dw_f32 over at most CK_MAX_RANGES row ranges, folded by papc_reduce_partials_strided_f32 into w's layout -- dY formed
//             on the fly from (dz, y) and the layer's BN constants in both.  New here: cck_colsum_kernel (per-cloud column sums of dY, per
//             128-row segment of a cloud) and cck_fold_kernel (segments in order, fold.h); dW_g, d bias and dg from s are cloud_concat.hip's
//             cc_tail_kernel, through cc_launch_tail.
// No float atomics, every cross-workgroup sum a fixed-order fold: two runs are bit-identical.  The small per-cloud products are fmaf chains in
// ascending index order.  Plain C++ loads and stores; every k loop is straight-line (operands always loaded from addresses that exist, then
// selected) and cck_drain holds the accumulators over the last MFMA's passes in front of the epilogue.
#include "carve.h"
#include "cloud_concat.h"

namespace papc {

constexpr int CK_BM = CC_BM;         // rows per forward tile / per column-sum segment
constexpr int CK_KS = 32;            // floats of K per forward stage
constexpr int CK_LD = 36;            // LDS pitch (floats) of a stage's rows: 16-byte aligned, 4 banks off per row
constexpr int CK_MAX_RANGES = 64;    // row ranges of the dW_p partials (each a [Cout, Cp] block: at most 32 MB at Cp = 256, Cout = 512)

__device__ __forceinline__ void ck_ld8(const float *p, float (&v)[8])
{
    const float4 a = ld4(p), b = ld4(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void cck_drain(floatx16 &acc) { asm volatile("s_nop 15" : "+a"(acc)); }

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// y tile [128 rows, BN columns] = x . W_p^T + c[b(row)].  BN = 128: 2 x 2 waves of 64 x 64 (2 x 2 MFMA blocks); BN = 64: 4 x 1 waves of 32 x 64.
// Workgroup blockIdx.x = row tile * (Cout / BN) + column block (the column blocks of a row tile run next to each other: x is read from HBM once).
template <int BN>
__global__ __launch_bounds__(CC_T) void cck_fwd_kernel(const float *__restrict__ x, int64_t ldx, const float *__restrict__ w, int64_t ldw,
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
    for (int i = 0; i < 4; ++i) xr[i] = ld4(xp[i]);
#pragma unroll
    for (int i = 0; i < NWR; ++i) wr[i] = ld4(wp + (int64_t)(32 * i) * ldw);
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
        for (int i = 0; i < 4; ++i) st4(&xs[(sr + 32 * i) * CK_LD + sq], xlive[i] ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f));
#pragma unroll
        for (int i = 0; i < NWR; ++i) st4(&ws[(sr + 32 * i) * CK_LD + sq], wr[i]);
        __syncthreads();
        const int kn = min(k0 + CK_KS, Cp - CK_KS);  // the next stage in flight over this one's products (the last stage re-reads itself)
#pragma unroll
        for (int i = 0; i < 4; ++i) xr[i] = ld4(xp[i] + kn);
#pragma unroll
        for (int i = 0; i < NWR; ++i) wr[i] = ld4(wp + (int64_t)(32 * i) * ldw + kn);
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
    cc_fwd_epilogue<IB, WMW, BN>(acc, red, cvec, wm, wn, tile, m0, n0, M, N, Cout, y, stats);
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// wt[k][o] = w[o][k], k < Cp: the operand papc_mlp_bwd_dx_f32 takes
__global__ __launch_bounds__(CC_T) void cck_wt_kernel(const float *__restrict__ w, int64_t ldw, int Cp, int Cout, float *__restrict__ wt)
{
    const int t = blockIdx.x * CC_T + threadIdx.x;
    if (t >= Cp * Cout) return;
    const int k = t / Cout, o = t - k * Cout;
    wt[t] = w[(int64_t)o * ldw + k];
}

// partial column sums of dY over segment blockIdx.x (128 rows) of cloud blockIdx.y: thread = (four columns, row group); a row group walks its
// rows in ascending order, the groups are added in order
__global__ __launch_bounds__(CC_T) void cck_colsum_kernel(const float *__restrict__ dz, const float *__restrict__ yv, const float *__restrict__ mean,
                                                          const float *__restrict__ invstd, const float *__restrict__ scale, const float *__restrict__ shift,
                                                          const float *__restrict__ c1, const float *__restrict__ c2, int N, int Cout,
                                                          float *__restrict__ part_s)
{
    __shared__ float4 red[CC_T];
    const int tid = threadIdx.x;
    const int ncq = Cout / 4, nrg = CC_T / ncq;
    const int cq = tid % ncq, rg = tid / ncq;
    const int b = blockIdx.y, n0 = blockIdx.x * CK_BM;
    const int rows = min(CK_BM, N - n0);
    const int64_t mr0 = (int64_t)b * N + n0;
    const int o = cq * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rg < nrg) {
        const float4 sc = ld4(scale + o), sh = ld4(shift + o), mu = ld4(mean + o), is = ld4(invstd + o), k1 = ld4(c1 + o), k2 = ld4(c2 + o);
        for (int r = rg; r < rows; r += nrg) {
            const float4 zz = ld4(dz + (mr0 + r) * Cout + o), yy = ld4(yv + (mr0 + r) * Cout + o);
            float4 d;
            cc_dy4(d, zz, yy, sc, sh, mu, is, k1, k2);
            a = fold_add(a, d);
        }
    }
    red[tid] = a;
    __syncthreads();
    if (rg == 0) {
        for (int t = 1; t < nrg; ++t) a = fold_add(a, red[t * ncq + cq]);
        st4(part_s + ((int64_t)b * gridDim.x + blockIdx.x) * Cout + o, a);
    }
}

// s[b][o] = sum over cloud b's nseg segments, in order from 0.f (fold.h)
__global__ __launch_bounds__(CC_T) void cck_fold_kernel(const float *__restrict__ part_s, int B, int nseg, int Cout, float *__restrict__ s)
{
    cc_fold_s(part_s, B, nseg, Cout, (int64_t)blockIdx.x * CC_T + threadIdx.x, s);
}

// dx[m][k] (+)= t[m][k]: the dense dX of papc_mlp_bwd_dx_f32 into a strided or accumulating destination
__global__ __launch_bounds__(CC_T) void cck_rows_out_kernel(const float *__restrict__ t, int64_t M, int Cp, float *__restrict__ dx, int64_t ldd, int accumulate)
{
    const int64_t e = (int64_t)blockIdx.x * CC_T + threadIdx.x;
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
    return cc_range_ok(who, B, N);
}

// rows per dW_p range: at most CK_MAX_RANGES ranges, whole multiples of 64 rows, at least 256
static int64_t cck_rows_per_range(int64_t M) { return std::max<int64_t>(256, cdiv(cdiv(M, CK_MAX_RANGES), 64) * 64); }

// workspace of the backward: [W_p^T | dW_p range partials | column-sum partials per segment | s | dense dX]
struct CckWs { float *wt, *part, *part_s, *s, *dxt; int64_t part_ld, ranges, rpr; };

static size_t cck_layout(int B, int N, int Cp, int Cout, void *base, CckWs &l)
{
    WsCarver c{static_cast<char *>(base), 0, 16};
    const int64_t M = (int64_t)B * N;
    l.rpr = cck_rows_per_range(M);
    l.ranges = cdiv(M, l.rpr);
    l.part_ld = (int64_t)Cout * Cp + Cout;
    l.wt = c.take<float>((size_t)Cp * Cout); l.part = c.take<float>((size_t)(l.ranges * l.part_ld));
    l.part_s = c.take<float>((size_t)B * cdiv(N, CK_BM) * Cout); l.s = c.take<float>((size_t)B * Cout);
    l.dxt = c.take<float>((size_t)M * Cp);
    return c.off;
}

}  // namespace papc

using namespace papc;

extern "C" {

int papc_cloud_concat_k_ok(int Cp, int Cg, int Cout) { return cck_widths_ok(Cp, Cg, Cout) ? 1 : 0; }

int papc_cloud_concat_k_parts(int B, int N) { return cc_parts(B, N); }

int papc_cloud_concat_k_f32(const float *x, int64_t ldx, const float *g, const float *w, const float *bias, int B, int N, int Cp, int Cg, int Cout,
                            float *y, float *cvec, float *stats_partial, papc_stream_t stream)
{
    const int err = cc_fwd_args_ok("papc_cloud_concat_k_f32", cck_shape_ok, x, ldx, g, w, B, N, Cp, Cg, Cout, y, cvec);
    if (err != PAPC_OK) return err;
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    const int64_t ldw = (int64_t)Cp + Cg;
    const int M = B * N;
    cc_launch_cvec(st, g, w, ldw, bias, B, Cp, Cg, Cout, cvec);
    const int e = check_launch("papc_cloud_concat_k_f32: c");
    if (e != PAPC_OK) return e;
    const int64_t tiles = cdiv(M, CK_BM);
    if (Cout % 128 == 0)
        hipLaunchKernelGGL(cck_fwd_kernel<128>, dim3((unsigned)(tiles * (Cout / 128))), dim3(CC_T), 0, st, x, ldx, w, ldw, cvec, M, N, Cp, Cout, y,
                           stats_partial);
    else
        hipLaunchKernelGGL(cck_fwd_kernel<64>, dim3((unsigned)(tiles * (Cout / 64))), dim3(CC_T), 0, st, x, ldx, w, ldw, cvec, M, N, Cp, Cout, y,
                           stats_partial);
    return check_launch("papc_cloud_concat_k_f32");
}

size_t papc_cloud_concat_k_bwd_workspace(int B, int N, int Cp, int Cg, int Cout)
{
    if (B < 1 || N < 1 || B > 65535 || (int64_t)B * N > ((int64_t)1 << 30) || !cck_widths_ok(Cp, Cg, Cout)) return 0;
    CckWs l;
    return cck_layout(B, N, Cp, Cout, nullptr, l);
}

int papc_cloud_concat_k_bwd_f32(const float *dz, const float *y, const float *mean, const float *invstd, const float *scale, const float *shift,
                                const float *c1, const float *c2, const float *x, int64_t ldx, const float *g, const float *w, int B, int N, int Cp,
                                int Cg, int Cout, float *dx, int64_t ldd, int accumulate, float *dw, float *dbias, float *dg, float *s_out,
                                void *workspace, size_t workspace_bytes, papc_stream_t stream)
{
    const int err = cc_bwd_args_ok("papc_cloud_concat_k_bwd_f32", cck_shape_ok, dz, y, mean, invstd, scale, shift, c1, c2, x, ldx, g, w, B, N, Cp, Cg, Cout,
                                   dx, ldd, dw, workspace, aligned16(workspace));
    if (err != PAPC_OK) return err;
    CckWs l;
    const size_t need = cck_layout(B, N, Cp, Cout, workspace, l);
    PAPC_REQUIRE(workspace_bytes >= need, PAPC_E_INVALID, "papc_cloud_concat_k_bwd_f32: workspace %zu bytes < %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const int64_t ldw = (int64_t)Cp + Cg;
    const int64_t M = (int64_t)B * N;
    const int nseg = (int)cdiv(N, CK_BM);
    float *s = s_out ? s_out : l.s;
    int e;
    {
        ProfScope prof(PAPC_K_MISC, st);
        hipLaunchKernelGGL(cck_colsum_kernel, dim3((unsigned)nseg, (unsigned)B), dim3(CC_T), 0, st, dz, y, mean, invstd, scale, shift, c1, c2, N, Cout,
                           l.part_s);
        e = check_launch("papc_cloud_concat_k_bwd_f32: column sums");
        if (e != PAPC_OK) return e;
        hipLaunchKernelGGL(cck_fold_kernel, dim3((unsigned)cdiv((int64_t)B * Cout, CC_T)), dim3(CC_T), 0, st, l.part_s, B, nseg, Cout, s);
        e = check_launch("papc_cloud_concat_k_bwd_f32: fold");
        if (e != PAPC_OK) return e;
        if (dx) {
            hipLaunchKernelGGL(cck_wt_kernel, dim3((unsigned)cdiv((int64_t)Cp * Cout, CC_T)), dim3(CC_T), 0, st, w, ldw, Cp, Cout, l.wt);
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
        e = papc_mlp_bwd_dx_f32(&dy, l.wt, M, Cp, Cout, direct ? dx : l.dxt, nullptr, nullptr, stream);
        if (e != PAPC_OK) return e;
        if (!direct) {
            ProfScope prof(PAPC_K_MISC, st);
            hipLaunchKernelGGL(cck_rows_out_kernel, dim3((unsigned)cdiv(M * Cp, CC_T)), dim3(CC_T), 0, st, l.dxt, M, Cp, dx, ldd, accumulate);
            e = check_launch("papc_cloud_concat_k_bwd_f32: dX rows");
            if (e != PAPC_OK) return e;
        }
    }
    e = papc_mlp_bwd_dw_f32(&dy, PAPC_A_PLAIN, x, ldx, nullptr, nullptr, nullptr, M, Cp, Cout, (int)l.rpr, l.part, l.part + (int64_t)Cout * Cp, l.part_ld, stream);
    if (e != PAPC_OK) return e;
    e = papc_reduce_partials_strided_f32(l.part, (int)l.ranges, l.part_ld, Cout, Cp, dw, ldw, 0, stream);
    if (e != PAPC_OK) return e;
    ProfScope prof(PAPC_K_MISC, st);
    cc_launch_tail(st, s, g, w, ldw, B, Cp, Cg, Cout, dw, dbias, dg);
    return check_launch("papc_cloud_concat_k_bwd_f32: tail");
}

}  // extern "C"
