// cloud_transform.hip -- the per-cloud transform of the T-Net PointNet classifier, for gfx950.
//
// Reference: /root/reference/PAPC/models/classify/pointnet/pointnet_Conv1D.py:85-88 (input transform, C = 3) and :96-99 (feature
// transform, C = 64):  y[b, n, :] = x[b, n, :] . T[b]   with T [B, C, C] row-major, one learned matrix per cloud.
//
//   forward   one launch: a workgroup owns a tile of one cloud's rows and stages T[b] (and for C = 64 the x tile) in LDS.
//   backward  dX[b] = dY[b] . T[b]^T and dT[b] = X[b]^T . dY[b] from ONE pass over dY: the N rows of a cloud are split into chunks (at
//             B = 32 there are too few clouds to fill the chip), each chunk writes its dX rows and its partial dT to a workspace slot of
//             its own; a second launch folds the chunks' partials in chunk order (fold.h).  No float atomics: two runs are bit-identical.
// Arithmetic is plain fp32 VALU (the operands are tiny; the launches are latency-sized): every output is a k-ordered fmaf chain from
// zero, compiled with -ffp-contract=off.  Plain C++ loads and stores only.
#include "fold.h"

namespace papc {

constexpr int CT_T = 256;       // threads of every kernel here (4 waves)
constexpr int CT_R64 = 64;      // rows per tile for C = 64
constexpr int CT_R3 = CT_T;     // rows per tile for C = 3 (one row per thread)

static inline int ct_rows(int C) { return C == 64 ? CT_R64 : CT_R3; }

// ---- C = 64 -------------------------------------------------------------------------------------------------------------------------
// thread: column j = lane, rows w + 4k (k < 16; w = wave, uniform across the wave -> the x tile reads are LDS broadcasts)
__global__ __launch_bounds__(CT_T) void ct_fwd64_kernel(const float *__restrict__ x, int64_t sb, int64_t sn, int64_t sc, const float *__restrict__ T,
                                                        int64_t ldt, int N, float *__restrict__ y)
{
    __shared__ float ts[64 * 64];
    __shared__ float xs[CT_R64 * 64];
    const int b = blockIdx.y, n0 = blockIdx.x * CT_R64, tid = threadIdx.x;
    const float *Tb = T + (int64_t)b * ldt;
    const float *xb = x + (int64_t)b * sb;
    for (int e = tid; e < 4096; e += CT_T) ts[e] = Tb[e];
    for (int e = tid; e < CT_R64 * 64; e += CT_T) {
        const int r = e >> 6, i = e & 63, n = n0 + r;
        xs[e] = n < N ? xb[(int64_t)n * sn + (int64_t)i * sc] : 0.f;
    }
    __syncthreads();
    const int j = tid & 63, w = tid >> 6;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.f;
    for (int i = 0; i < 64; ++i) {
        const float t = ts[i * 64 + j];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = fmaf(xs[(w + 4 * k) * 64 + i], t, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int n = n0 + w + 4 * k;
        if (n < N) y[((int64_t)b * N + n) * 64 + j] = acc[k];
    }
}

// chunk = blockIdx.x: dX rows of the chunk and the chunk's partial dT [64, 64] -> part[(b * nch + chunk) * 4096 ..]
__global__ __launch_bounds__(CT_T) void ct_bwd64_kernel(const float *__restrict__ x, int64_t sb, int64_t sn, int64_t sc, const float *__restrict__ T,
                                                        int64_t ldt, const float *__restrict__ dy, int N, float *dx, int64_t dsb, int64_t dsn, int64_t dsc,
                                                        int accumulate, float *__restrict__ part)
{
    __shared__ float ts[64 * 65];       // T[i][j] at i * 65 + j: the dX pass reads column-wise (lane = i), pitch 65 keeps it conflict-free
    __shared__ float xs[CT_R64 * 64];
    __shared__ float gs[CT_R64 * 64];
    const int b = blockIdx.y, chunk = blockIdx.x, n0 = chunk * CT_R64, tid = threadIdx.x;
    const float *Tb = T + (int64_t)b * ldt;
    const float *xb = x + (int64_t)b * sb;
    const float *gb = dy + (int64_t)b * N * 64;
    for (int e = tid; e < 4096; e += CT_T) ts[(e >> 6) * 65 + (e & 63)] = Tb[e];
    for (int e = tid; e < CT_R64 * 64; e += CT_T) {
        const int r = e >> 6, i = e & 63, n = n0 + r;
        const bool ok = n < N;
        xs[e] = ok ? xb[(int64_t)n * sn + (int64_t)i * sc] : 0.f;
        gs[e] = ok ? gb[(int64_t)n * 64 + i] : 0.f;
    }
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6;
    float acc[16];
    if (dx) {                           // dX[r][i] = sum_j dY[r][j] T[i][j]   (lane = i)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.f;
        for (int jj = 0; jj < 64; ++jj) {
            const float t = ts[lane * 65 + jj];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] = fmaf(gs[(w + 4 * k) * 64 + jj], t, acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int n = n0 + w + 4 * k;
            if (n < N) {
                float *p = dx + (int64_t)b * dsb + (int64_t)n * dsn + (int64_t)lane * dsc;
                *p = accumulate ? *p + acc[k] : acc[k];
            }
        }
    }
    // partial dT[i][j] = sum_r X[r][i] dY[r][j]   (lane = j, i = w + 4k; rows past N are zero in both tiles)
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.f;
    for (int r = 0; r < CT_R64; ++r) {
        const float g = gs[r * 64 + lane];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = fmaf(xs[r * 64 + w + 4 * k], g, acc[k]);
    }
    float *pp = part + ((int64_t)b * gridDim.x + chunk) * 4096;
#pragma unroll
    for (int k = 0; k < 16; ++k) pp[(w + 4 * k) * 64 + lane] = acc[k];
}

// ---- C = 3 --------------------------------------------------------------------------------------------------------------------------
// one row per thread; T[b] (9 floats) is read by every thread of the workgroup (one cache line)
__global__ __launch_bounds__(CT_T) void ct_fwd3_kernel(const float *__restrict__ x, int64_t sb, int64_t sn, int64_t sc, const float *__restrict__ T,
                                                       int64_t ldt, int N, float *__restrict__ y)
{
    const int b = blockIdx.y, n = blockIdx.x * CT_R3 + threadIdx.x;
    if (n >= N) return;
    const float *Tb = T + (int64_t)b * ldt;
    const float *p = x + (int64_t)b * sb + (int64_t)n * sn;
    const float x0 = p[0], x1 = p[sc], x2 = p[2 * sc];
    float *o = y + ((int64_t)b * N + n) * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = fmaf(x2, Tb[6 + j], fmaf(x1, Tb[3 + j], fmaf(x0, Tb[j], 0.f)));
}

__global__ __launch_bounds__(CT_T) void ct_bwd3_kernel(const float *__restrict__ x, int64_t sb, int64_t sn, int64_t sc, const float *__restrict__ T,
                                                       int64_t ldt, const float *__restrict__ dy, int N, float *dx, int64_t dsb, int64_t dsn, int64_t dsc,
                                                       int accumulate, float *__restrict__ part)
{
    __shared__ float red[9][CT_T];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x, n = chunk * CT_R3 + tid;
    const bool ok = n < N;
    float xv[3] = {0.f, 0.f, 0.f}, gv[3] = {0.f, 0.f, 0.f};
    if (ok) {
        const float *p = x + (int64_t)b * sb + (int64_t)n * sn;
        const float *g = dy + ((int64_t)b * N + n) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) { xv[i] = p[i * sc]; gv[i] = g[i]; }
    }
    const float *Tb = T + (int64_t)b * ldt;
    if (dx && ok) {                     // dX[i] = sum_j dY[j] T[i][j]
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float v = fmaf(gv[2], Tb[3 * i + 2], fmaf(gv[1], Tb[3 * i + 1], fmaf(gv[0], Tb[3 * i], 0.f)));
            float *q = dx + (int64_t)b * dsb + (int64_t)n * dsn + (int64_t)i * dsc;
            *q = accumulate ? *q + v : v;
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) red[3 * i + j][tid] = xv[i] * gv[j];
    __syncthreads();
    for (int s = CT_T / 2; s > 0; s >>= 1) {      // fixed tree over the workgroup's rows
        if (tid < s) {
#pragma unroll
            for (int e = 0; e < 9; ++e) red[e][tid] += red[e][tid + s];
        }
        __syncthreads();
    }
    if (tid < 9) part[((int64_t)b * gridDim.x + chunk) * 9 + tid] = red[tid][0];
}

// ---- the fold: dT[b][e] = sum over chunks c of part[b][c][e] (fold.h: in order from the first chunk) ---------------------------------------
__global__ __launch_bounds__(CT_T) void ct_fold_kernel(const float *__restrict__ part, int nch, int CC, int64_t total, float *__restrict__ dT)
{
    const int64_t t = (int64_t)blockIdx.x * CT_T + threadIdx.x;
    if (t >= total) return;
    const int64_t b = t / CC, e = t - b * CC;
    dT[t] = fold_in_order<1, FOLD_FROM_FIRST, float>(part, CC, nch, b * nch * CC + e);
}

}  // namespace papc

using namespace papc;

extern "C" {

size_t papc_cloud_transform_bwd_workspace(int B, int N, int C)
{
    if (B < 1 || N < 1 || (C != 3 && C != 64)) return 0;
    return (size_t)B * (size_t)cdiv(N, ct_rows(C)) * (size_t)C * (size_t)C * sizeof(float);
}

int papc_cloud_transform_f32(const float *x, int64_t sb, int64_t sn, int64_t sc, const float *T, int64_t ldt, int B, int N, int C, float *y,
                             papc_stream_t stream)
{
    PAPC_REQUIRE(x && T && y, PAPC_E_INVALID, "papc_cloud_transform_f32: null pointer");
    PAPC_REQUIRE(C == 3 || C == 64, PAPC_E_UNSUPPORTED, "papc_cloud_transform_f32: C=%d (3 or 64)", C);
    PAPC_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && ldt >= (int64_t)C * C, PAPC_E_INVALID, "papc_cloud_transform_f32: B=%d N=%d ldt=%lld", B, N, (long long)ldt);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    if (C == 64) hipLaunchKernelGGL(ct_fwd64_kernel, dim3((unsigned)cdiv(N, CT_R64), (unsigned)B), dim3(CT_T), 0, st, x, sb, sn, sc, T, ldt, N, y);
    else hipLaunchKernelGGL(ct_fwd3_kernel, dim3((unsigned)cdiv(N, CT_R3), (unsigned)B), dim3(CT_T), 0, st, x, sb, sn, sc, T, ldt, N, y);
    return check_launch("papc_cloud_transform_f32");
}

int papc_cloud_transform_bwd_f32(const float *x, int64_t sb, int64_t sn, int64_t sc, const float *T, int64_t ldt, const float *dy, int B, int N, int C,
                                 float *dx, int64_t dsb, int64_t dsn, int64_t dsc, int accumulate, float *dT, void *workspace,
                                 size_t workspace_bytes, papc_stream_t stream)
{
    PAPC_REQUIRE(x && T && dy && dT && workspace, PAPC_E_INVALID, "papc_cloud_transform_bwd_f32: null pointer");
    PAPC_REQUIRE(C == 3 || C == 64, PAPC_E_UNSUPPORTED, "papc_cloud_transform_bwd_f32: C=%d (3 or 64)", C);
    PAPC_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && ldt >= (int64_t)C * C, PAPC_E_INVALID, "papc_cloud_transform_bwd_f32: B=%d N=%d ldt=%lld", B, N, (long long)ldt);
    const size_t need = papc_cloud_transform_bwd_workspace(B, N, C);
    PAPC_REQUIRE(workspace_bytes >= need, PAPC_E_INVALID, "papc_cloud_transform_bwd_f32: workspace %zu bytes < %zu", workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    float *part = static_cast<float *>(workspace);
    const int nch = (int)cdiv(N, ct_rows(C));
    if (C == 64)
        hipLaunchKernelGGL(ct_bwd64_kernel, dim3((unsigned)nch, (unsigned)B), dim3(CT_T), 0, st, x, sb, sn, sc, T, ldt, dy, N, dx, dsb, dsn, dsc, accumulate, part);
    else
        hipLaunchKernelGGL(ct_bwd3_kernel, dim3((unsigned)nch, (unsigned)B), dim3(CT_T), 0, st, x, sb, sn, sc, T, ldt, dy, N, dx, dsb, dsn, dsc, accumulate, part);
    const int err = check_launch("papc_cloud_transform_bwd_f32");
    if (err != PAPC_OK) return err;
    const int64_t total = (int64_t)B * C * C;
    hipLaunchKernelGGL(ct_fold_kernel, dim3((unsigned)cdiv(total, CT_T)), dim3(CT_T), 0, st, part, nch, C * C, total, dT);
    return check_launch("papc_cloud_transform_bwd_f32: fold");
}

}  // extern "C"
