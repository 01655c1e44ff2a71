// finalize.h -- the closed-form finalizes that need no launch of their own, written once.  The two of the backward (the no-store max layer's
// dW, the coordinates-only first layer's gradients) run as launches (mlp_dw.hip, xyz1.hip) or as workgroups of papc_fold_jobs_f32's finalize
// launch (folds.hip, fold_fin_kernel); the first layer's forward finalize as a launch (xyz1.hip) or as one workgroup of the step's weight
// transposes (bn_ops.hip).  The same arithmetic per output element either way: the results are bit-identical.
#pragma once
#include "common.h"

namespace papc {

constexpr int DWMAX_CI = 64;
constexpr int DWMAX_FIN_LDS = DWMAX_CI * DWMAX_CI;       // doubles of LDS per workgroup
constexpr int XYZ_BWD_FIN_LDS = 64 * 17 + 8 * 17;

// dW[c, i] = T[c, i] - sc_c c1_c S_i - e_c sum_j W[c, j] (G[j, i] - S_j S_i / M); four rows of dW per workgroup `wg`: every thread of the
// workgroup (nt of them, >= 256) helps to centre the Gram block, the first 256 form the rows.  gc: DWMAX_FIN_LDS doubles.
__device__ __forceinline__ void dw_max_finalize_body(double *__restrict__ gc, int wg, int nt, const double *__restrict__ fold, const float *__restrict__ w,
                                                     const float *__restrict__ e, const float *__restrict__ scale, const float *__restrict__ c1, double inv_m,
                                                     int Cout, float *__restrict__ dw, int accumulate)
{
    constexpr int CI = DWMAX_CI;
    const int tid = threadIdx.x;
    const double *G = fold + (int64_t)Cout * CI, *S = G + CI * CI;
    for (int q = tid; q < CI * CI; q += nt) {
        const int j = q >> 6, i = q & 63;
        gc[j * CI + i] = G[q] - S[j] * S[i] * inv_m;
    }
    __syncthreads();
    const int i = tid & 63, c = 4 * wg + (tid >> 6);
    if (tid >= 256 || c >= Cout) return;
    double dot = 0.0;
    for (int j = 0; j < CI; ++j) dot += (double)w[(int64_t)c * CI + j] * gc[j * CI + i];
    const double v = fold[(int64_t)c * CI + i] - (double)scale[c] * (double)c1[c] * S[i] - (double)e[c] * dot;
    float *o = dw + (int64_t)c * CI + i;
    *o = accumulate ? *o + (float)v : (float)v;
}

// The coordinates-only first layer's forward finalize: moments [parts][16] -> gram[16] (fixed order), then per channel the BatchNorm constants
// and the folded first layer.  One workgroup of 256 threads; a launch of its own (xyz1.hip) or one extra workgroup of the step's weight
// transposes (bn_ops.hip).  red: 16 * 16 + 10 doubles.
struct XyzL1Fin {
    const double *partial; int parts; double M;
    const float *w; int ldw, xcol0;
    const float *bias, *gamma, *beta;
    float eps, momentum; int C;
    float *mean, *invstd, *scale, *shift, *rmean, *rvar, *wf;
    double *gram;
};
constexpr int XYZ_L1_FIN_LDS = 16 * 16 + 10;
// (bn_ops.hip) `count` in [0, 8] weight transposes (papc_transpose_batch_ld_f32's arguments) with this finalize as one extra workgroup
int transpose_batch_l1(const float *const *src, const int *src_ld, float *const *dst, const int *rows, const int *cols, const int *copy, int count,
                       const XyzL1Fin &a, hipStream_t st);
__device__ __forceinline__ void xyz_l1_finalize_body(double *__restrict__ lds, const XyzL1Fin &a)
{
    double(*red)[16] = reinterpret_cast<double(*)[16]>(lds);
    double *G = lds + 16 * 16;
    const double M = a.M;
    const int e = threadIdx.x & 15, sl = threadIdx.x >> 4;      // 16 entries (10 used) x 16 slices
    double s = 0.0;
    if (e < 10) for (int t = sl; t < a.parts; t += 16) s += a.partial[(int64_t)t * 16 + e];
    red[sl][e] = s;
    __syncthreads();
    if (threadIdx.x < 10) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) v += red[q][threadIdx.x];
        G[threadIdx.x] = v;
        a.gram[threadIdx.x] = v;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < a.C; c += 256) {
        const double w0 = a.w[(int64_t)c * a.ldw + a.xcol0], w1 = a.w[(int64_t)c * a.ldw + a.xcol0 + 1], w2 = a.w[(int64_t)c * a.ldw + a.xcol0 + 2];
        const double b = a.bias ? (double)a.bias[c] : 0.0;
        const double mx = G[0] / M, my = G[1] / M, mz = G[2] / M;
        // covariance of the inputs (biased), then the variance of y = W x + b: W Cov W^T
        const double cxx = G[3] / M - mx * mx, cxy = G[4] / M - mx * my, cxz = G[5] / M - mx * mz;
        const double cyy = G[6] / M - my * my, cyz = G[7] / M - my * mz, czz = G[8] / M - mz * mz;
        const double mu = w0 * mx + w1 * my + w2 * mz + b;
        double var = w0 * (w0 * cxx + w1 * cxy + w2 * cxz) + w1 * (w0 * cxy + w1 * cyy + w2 * cyz) + w2 * (w0 * cxz + w1 * cyz + w2 * czz);
        if (var < 0.0) var = 0.0;
        const double is = 1.0 / sqrt(var + (double)a.eps);
        const double sc = (a.gamma ? (double)a.gamma[c] : 1.0) * is;
        const double sh = (a.beta ? (double)a.beta[c] : 0.0) - mu * sc;
        a.mean[c] = (float)mu; a.invstd[c] = (float)is; a.scale[c] = (float)sc; a.shift[c] = (float)sh;
        if (a.rmean) a.rmean[c] = a.momentum * a.rmean[c] + (1.f - a.momentum) * (float)mu;     // paddle: momentum weighs the running value
        if (a.rvar) a.rvar[c] = a.momentum * a.rvar[c] + (1.f - a.momentum) * (float)var;
        // a = relu(scale (W x + b) + shift) = relu(wf . x + t)
        a.wf[c * 4 + 0] = (float)(sc * w0); a.wf[c * 4 + 1] = (float)(sc * w1); a.wf[c * 4 + 2] = (float)(sc * w2);
        a.wf[c * 4 + 3] = (float)(sc * b + sh);
    }
}

// partial [parts][C][4] (T0, T1, T2, S) + the input moments -> dgamma, dbeta, dW [C][3]  (closed form, float64).
// A workgroup of 1024 threads owns 4 channels: 16 entries x 64 slices of the partial rows, summed in fixed order.  The kernel is one latency
// chain: with 64 slices a thread's share of <= 768 partial rows is 12 loads, all in flight at once -- one memory round trip instead of six
// (17.6 -> ~7 us in the replayed step).  lds: XYZ_BWD_FIN_LDS doubles.
__device__ __forceinline__ void xyz_l1_bwd_finalize_body(double *__restrict__ lds, int wg, const float *__restrict__ partial, int parts, double M, int C,
                                                         const double *__restrict__ gram, const float *__restrict__ w, int ldw, int xcol0,
                                                         const float *__restrict__ bias, const float *__restrict__ mean, const float *__restrict__ invstd,
                                                         const float *__restrict__ scale, float *dgamma, float *dbeta, float *dw, int accumulate)
{
    double(*red)[17] = reinterpret_cast<double(*)[17]>(lds);
    double(*red2)[17] = reinterpret_cast<double(*)[17]>(lds + 64 * 17);
    const int e = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int e0 = wg * 16;                          // first entry (channel * 4 + slot) of this workgroup
    const int c = wg * 4 + threadIdx.x;
    const bool fin = threadIdx.x < 4 && c < C;       // (the finalizing threads fetch their constants with the partial rows, not behind the barriers)
    const int cc = fin ? c : 0;
    const double w0 = w[(int64_t)cc * ldw + xcol0], w1 = w[(int64_t)cc * ldw + xcol0 + 1], w2 = w[(int64_t)cc * ldw + xcol0 + 2];
    const double b = bias ? (double)bias[cc] : 0.0;
    const double mu = mean[cc], is = invstd[cc], sc = scale[cc];
    double gq[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) gq[i] = gram[i];
    double s = 0.0;
    if (e0 + e < C * 4) {
        for (int t0 = sl; t0 < parts; t0 += 64 * 12) {   // 12 loads in flight per thread
            float v[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) v[q] = (t0 + 64 * q < parts) ? partial[(int64_t)(t0 + 64 * q) * C * 4 + e0 + e] : 0.f;
#pragma unroll
            for (int q = 0; q < 12; ++q) s += (double)v[q];
        }
    }
    red[sl][e] = s;
    __syncthreads();
    if (sl < 8) {                                    // 64 slices -> 8 -> 1, fixed order
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += red[sl * 8 + q][e];
        red2[sl][e] = t;
    }
    __syncthreads();
    if (sl == 0) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += red2[q][e];
        red[0][e] = t;
    }
    __syncthreads();
    if (fin) {
        const double T0 = red[0][threadIdx.x * 4 + 0], T1 = red[0][threadIdx.x * 4 + 1], T2 = red[0][threadIdx.x * 4 + 2], S = red[0][threadIdx.x * 4 + 3];
        const double dg = is * (w0 * T0 + w1 * T1 + w2 * T2 + (b - mu) * S);     // sum p xhat
        dbeta[c] = accumulate ? dbeta[c] + (float)S : (float)S;
        dgamma[c] = accumulate ? dgamma[c] + (float)dg : (float)dg;
        const double c1 = S / M, c2 = dg / M;
        const double Sx[3] = {gq[0], gq[1], gq[2]};
        const double Sxx[3][3] = {{gq[3], gq[4], gq[5]}, {gq[4], gq[6], gq[7]}, {gq[5], gq[7], gq[8]}};
        const double T[3] = {T0, T1, T2};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double yx = w0 * Sxx[0][k] + w1 * Sxx[1][k] + w2 * Sxx[2][k] + (b - mu) * Sx[k];      // sum_m (y - mean) x_k
            const float gk_ = (float)(sc * (T[k] - c1 * Sx[k] - c2 * is * yx));
            float *o = dw + (int64_t)c * ldw + xcol0 + k;
            *o = accumulate ? *o + gk_ : gk_;
        }
    }
}

}  // namespace papc
