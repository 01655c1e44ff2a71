// kdbn.hip -- one down level of the KDUNet part segmenter, for gfx950: 1x1 conv to 3F channels, BatchNorm over all 3F channels, ReLU, the
// kd-tree select, the max over point pairs.
//
// Reference: PAPC/models/segment/kdunet/kdunet.py:51-61 (ConvBNReLU :20-39)
//     x = relu(batch_norm(conv(x)));  x = reshape(x, (-1, F, 3, dim));  x = reshape(x, (-1, F, 3 * dim));
//     x = index_select(x, axis=2, index=sel + 3 * arange(dim));  x = max(reshape(x, (-1, F, dim / 2, 2)), axis=-1)
// The select is kdconv.hip's: pre-pool row n takes channel 3f + k at source point p, and the kernels that walk it (forward, dX, dW and their
// Cin = 3 twins) run kdlevel.h's bodies, as kdconv.hip's do; this file hands in what the norm adds.  The BatchNorm statistics run over EVERY point
// and every one of the 3F channels, but the conv is linear in its input rows, so they follow from the moments of the Cin-wide rows
// x [M = B dim, Cin]:  xm = mean_n x[n],  C = sum_n (x[n] - xm)(x[n] - xm)^T,  T = W C  [3F, Cin]:
//     mu_c = w_c . xm + b_c     var_c = max(T_c . w_c / M, 0)     rstd_c = 1 / sqrt(var_c + eps)     r_c = gamma_c rstd_c
//     zhat_c[n] = (w_c . x[n] - w_c . xm) rstd_c     a = gamma zhat + beta     y = relu(a)     out[m, f] = max(y[2m], y[2m + 1])
// (the conv bias cancels out of a; it enters the running mean only).  Only the selected third of the conv is computed and the [M, 3F]
// activations are never formed, in either direction.  With g[n, c] = gout where (n, c) was selected, won its pair and out > 0, else 0:
//     dbeta_c = sum_n g_c[n]      dgamma_c = sum_n g_c[n] zhat_c[n]      S_c = sum_n g_c[n] x[p(n)]
//     dW_c = r_c (S_c - dbeta_c xm - (dgamma_c rstd_c / M) T_c)          d bias = 0
//     dX[n] = sum_c r_c g_c[n] w_c - v - (x[n] - xm) A       v = sum_c (r_c dbeta_c / M) w_c      A = W^T diag(r_c dgamma_c rstd_c / M) W
//
//   moments   kb_colsum_kernel: column sums of chunks of 256 rows; kb_mean_kernel folds them in chunk order (fold.h, in-order) -> xm.
//             kb_gram_kernel: the CENTRED second moment of a chunk (two passes over x: no cancellation), a wave per 32 x 32 block of C;
//             folded in chunk order by papc_reduce_partials_f32.  kb_t_kernel: T = W C (C's two triangles agree to rounding; the B operand
//             reads C by rows).  kb_finalize_kernel: a wave per channel, double sums -> zoff = w . xm, rstd, mu, var; running statistics
//             momentum * running + (1 - momentum) * batch, the biased variance (models._bn1d, bn_ops.hip).
//             Eval mode: kb_eval_kernel takes zoff = running_mean - bias, rstd from running_var; the forward kernel is the same.
//   forward   kb_fwd_kernel: kd_fwd_acc (kdlevel.h); epilogue zhat = (acc - zoff) rstd, a = gamma zhat + beta, ReLU, pair max.  Writes
//             out, the winner byte and the winner's zhat (the backward's dgamma needs it; it is never recovered by dividing by gamma).
//   backward  kb_dw_kernel: kd_dw_acc with two row sums -> per chunk S [3F, Cin], dbeta [3F], dgamma [3F]; folded in chunk order by
//             papc_reduce_partials2_f32.  kb_dwfin_kernel: dW, dgamma, dbeta (d bias = exact zeros, nothing under accumulate) and the
//             per-channel coefficients r, r dbeta / M, r dgamma rstd / M.  kb_a_kernel: A and v, a wave per 32 x 32 block and slice of the 3F
//             channels, the slices folded in slice order.  kb_dx_kernel: kd_dx_acc with dy = r g, then Cin more k steps (x - xm) (-A), minus v.
//             No float atomics, every sum in a fixed order: two runs are bit-identical.  In eval mode the norm is a fixed affine map:
//             dW_c = r_c S_c, d bias_c = r_c dbeta_c, dX is the sparse term alone.
// Products: bf16x3.h on v_mfma_f32_32x32x16_bf16 (fp32 accuracy, fp32 accumulation) for Cin >= 32; the Cin = 3 first level runs fmaf chains
// on the vector unit (the *3_kernel twins).  Plain C++ loads and stores only.
#include "carve.h"
#include "fold.h"
#include "kdlevel.h"

namespace papc {

constexpr int KB_T = KD_T;       // threads of every kernel here (4 waves)
constexpr int KB_MCH = 256;      // rows per moments chunk
constexpr int KB_FMAX = 1024;    // the widest level

// ---- moments ------------------------------------------------------------------------------------------------------------------------
// chunk t (blockIdx.x) = rows 256 t .. + 255; workgroup = 16 columns (blockIdx.y) x 16 slices of 16 rows, each summed in row order, the slices
// added in slice order: part[t * Cin + c]
__global__ __launch_bounds__(KB_T) void kb_colsum_kernel(const float *__restrict__ x, int64_t ldx, int M, int Cin, float *__restrict__ part)
{
    __shared__ float red[16][16];
    const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int c = blockIdx.y * 16 + cl;
    const int r0 = blockIdx.x * KB_MCH + sl * (KB_MCH / 16), r1 = min(r0 + KB_MCH / 16, M);
    float s = 0.f;
    if (c < Cin)
        for (int m = r0; m < r1; ++m) s += x[(int64_t)m * ldx + c];
    red[sl][cl] = s;
    __syncthreads();
    if (sl != 0 || c >= Cin) return;
#pragma unroll
    for (int g = 1; g < 16; ++g) s += red[g][cl];
    part[(int64_t)blockIdx.x * Cin + c] = s;
}

__global__ __launch_bounds__(KB_T) void kb_mean_kernel(const float *__restrict__ part, int T, int M, int Cin, float *__restrict__ mean)
{
    const int c = blockIdx.x * KB_T + threadIdx.x;
    if (c >= Cin) return;
    mean[c] = fold_in_order<8, FOLD_FROM_ZERO, float>(part, Cin, T, c) / (float)M;
}

// wave = block (cb1, cb2) of the chunk's centred second moment: A[row r = c1][n] = x[n][32 cb1 + r] - xm, B[n][col r] = x[n][32 cb2 + r] - xm
__global__ __launch_bounds__(KB_T) void kb_gram_kernel(const float *__restrict__ x, int64_t ldx, const float *__restrict__ mean, int M, int Cin,
                                                       float *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int ncb = Cin >> 5, id = blockIdx.y * 4 + wv;
    if (id >= ncb * ncb) return;
    const int cb1 = id / ncb, cb2 = id - cb1 * ncb;
    const int c1 = cb1 * 32 + r, c2 = cb2 * 32 + r;
    const float m1 = mean[c1], m2 = mean[c2];
    const int r0 = blockIdx.x * KB_MCH;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int ks = 0; ks < KB_MCH / 16; ++ks) {
        const int mb = r0 + ks * 16 + 8 * h;
        if (r0 + ks * 16 >= M) break;                               // (wave-uniform)
        float av[8], bv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = mb + j < M;
            const float *xr = x + (int64_t)(in ? mb + j : 0) * ldx;
            av[j] = in ? xr[c1] - m1 : 0.f;
            bv[j] = in ? xr[c2] - m2 : 0.f;
        }
        acc = kd_step(av, bv, acc);
    }
    float *pt = part + (int64_t)blockIdx.x * Cin * Cin;
#pragma unroll
    for (int i = 0; i < 16; ++i) pt[(int64_t)(cb1 * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * Cin + c2] = acc[i];
}

// Cin = 3: workgroup = the 9 elements (c1, c2) of the chunk's centred second moment x 16 slices of 16 rows, the slices added in slice order
__global__ __launch_bounds__(KB_T) void kb_gram3_kernel(const float *__restrict__ x, int64_t ldx, const float *__restrict__ mean, int M,
                                                        float *__restrict__ part)
{
    __shared__ float red[16][16];
    const int e = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int c1 = min(e / 3, 2), c2 = e % 3;
    const float m1 = mean[c1], m2 = mean[c2];
    const int r0 = blockIdx.x * KB_MCH + sl * (KB_MCH / 16), r1 = min(r0 + KB_MCH / 16, M);
    float s = 0.f;
    for (int m = r0; m < r1; ++m) {
        const float *xr = x + (int64_t)m * ldx;
        s = fmaf(xr[c1] - m1, xr[c2] - m2, s);
    }
    red[sl][e] = s;
    __syncthreads();
    if (sl != 0 || e >= 9) return;
#pragma unroll
    for (int g = 1; g < 16; ++g) s += red[g][e];
    part[(int64_t)blockIdx.x * 9 + e] = s;
}

// T = W C.  wave: channels 32 ob .. + 31 (blockIdx.x), columns 32 cb .. + 31: A[row r][c] = W[32 ob + r][c], B[c][col r] = C[32 cb + r][c]
__global__ __launch_bounds__(KB_T) void kb_t_kernel(const float *__restrict__ w, const float *__restrict__ cm, int Cin, float *__restrict__ tm)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int cb = blockIdx.y * 4 + wv;
    if (cb * 32 >= Cin) return;
    const int o0 = blockIdx.x * 32;
    const float *wr = w + (int64_t)(o0 + r) * Cin + 8 * h, *cr = cm + (int64_t)(cb * 32 + r) * Cin + 8 * h;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int c0 = 0; c0 < Cin; c0 += 16) {
        float av[8], bv[8];
        kd_ld8(wr + c0, av);
        kd_ld8(cr + c0, bv);
        acc = kd_step(av, bv, acc);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) tm[(int64_t)(o0 + (i & 3) + 8 * (i >> 2) + 4 * h) * Cin + cb * 32 + r] = acc[i];
}

__global__ __launch_bounds__(KB_T) void kb_t3_kernel(const float *__restrict__ w, const float *__restrict__ cm, int n_ch, float *__restrict__ tm)
{
    const int o = blockIdx.x * KB_T + threadIdx.x;
    if (o >= n_ch) return;
    const float w0 = w[3 * o], w1 = w[3 * o + 1], w2 = w[3 * o + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) tm[3 * o + c] = fmaf(w2, cm[6 + c], fmaf(w1, cm[3 + c], w0 * cm[c]));
}

// one wave per channel o: zoff = w_o . xm, var = T_o . w_o / M in double; stats = [zoff | rstd | mu | var] x [n_ch]
__global__ __launch_bounds__(64) void kb_finalize_kernel(const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ mean,
                                                         const float *__restrict__ tm, int M, int Cin, int n_ch, float eps, float momentum,
                                                         float *__restrict__ stats, float *rmean, float *rvar)
{
    const int o = blockIdx.x, tl = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int c = tl; c < Cin; c += 64) {
        const double wv = (double)w[(int64_t)o * Cin + c];
        s1 += wv * (double)mean[c];
        s2 += wv * (double)tm[(int64_t)o * Cin + c];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {                            // (a butterfly: every lane ends with the same sum, in a fixed order)
        s1 += __shfl_xor(s1, d);
        s2 += __shfl_xor(s2, d);
    }
    if (tl == 0) {
        double var = s2 / (double)M;                               // the biased variance (paddle BatchNorm training)
        if (!(var > 0.0)) var = var != var ? var : 0.0;
        const float mu = (float)(s1 + (bias ? (double)bias[o] : 0.0));
        stats[o] = (float)s1;
        stats[n_ch + o] = (float)(1.0 / sqrt(var + (double)eps));
        stats[2 * n_ch + o] = mu;
        stats[3 * n_ch + o] = (float)var;
        if (rmean) rmean[o] = momentum * rmean[o] + (1.f - momentum) * mu;   // paddle: momentum weighs the running value
        if (rvar) rvar[o] = momentum * rvar[o] + (1.f - momentum) * (float)var;
    }
}

__global__ __launch_bounds__(KB_T) void kb_eval_kernel(const float *__restrict__ bias, const float *__restrict__ rmean, const float *__restrict__ rvar,
                                                       int n_ch, float eps, float *__restrict__ stats)
{
    const int o = blockIdx.x * KB_T + threadIdx.x;
    if (o >= n_ch) return;
    const float mu = rmean[o], var = rvar[o];
    stats[o] = mu - (bias ? bias[o] : 0.f);
    stats[n_ch + o] = (float)(1.0 / sqrt((double)var + (double)eps));
    stats[2 * n_ch + o] = mu;
    stats[3 * n_ch + o] = var;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
struct KbChan { float zoff, rstd, gamma, beta; };

__device__ __forceinline__ KbChan kb_chan(const float *__restrict__ stats, const float *__restrict__ gamma, const float *__restrict__ beta, int n_ch, int o)
{
    return KbChan{stats[o], stats[n_ch + o], gamma[o], beta[o]};
}

// acc = w . x (no bias) -> zhat, a
__device__ __forceinline__ void kb_affine(float acc, const KbChan &c, float &z, float &a)
{
    z = (acc - c.zoff) * c.rstd;
    a = c.gamma * z + c.beta;
}

__device__ __forceinline__ void kb_store_pair(float z0, float a0, float z1, float a1, float *__restrict__ out, unsigned char *__restrict__ win,
                                              float *__restrict__ zh, int64_t at)
{
    const float y0 = relu_np(a0), y1 = relu_np(a1);
    const bool w1 = y1 > y0 || (y1 != y1 && y0 == y0);     // the first row on an exact tie; a NaN goes through, as the source's max does
    out[at] = w1 ? y1 : y0;
    win[at] = w1 ? 1 : 0;
    zh[at] = w1 ? z1 : z0;
}

// wave: rows m0 .. m0 + 31 (blockIdx.x), features 32 fb .. + 31 (fb = 4 blockIdx.y + wave): kd_fwd_acc, then per pair the norm, ReLU and max
__global__ __launch_bounds__(KB_T) void kb_fwd_kernel(const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss,
                                                      const float *__restrict__ w, const float *__restrict__ stats, const float *__restrict__ gamma,
                                                      const float *__restrict__ beta, int M, int dim, int Cin, int F, float *__restrict__ out,
                                                      unsigned char *__restrict__ win, float *__restrict__ zh)
{
    const int fb = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (fb * 32 >= F) return;
    const int m0 = blockIdx.x * 32, f = fb * 32 + (threadIdx.x & 31);
    int k;
    const floatx16 acc = kd_fwd_acc(x, ldx, sel, ss, w, M, dim, Cin, m0, f, k);
    const KbChan ch[3] = {kb_chan(stats, gamma, beta, 3 * F, 3 * f), kb_chan(stats, gamma, beta, 3 * F, 3 * f + 1), kb_chan(stats, gamma, beta, 3 * F, 3 * f + 2)};
    // (captured by value: by reference, ch is indexed through the closure and lands in scratch)
    kd_fwd_pairs(acc, k, m0, M, F, f, [=](float acc0, int k0, float acc1, int k1, int64_t at) {
        float z0, a0, z1, a1;
        kb_affine(acc0, k0 == 0 ? ch[0] : (k0 == 1 ? ch[1] : ch[2]), z0, a0);
        kb_affine(acc1, k1 == 0 ? ch[0] : (k1 == 1 ? ch[1] : ch[2]), z1, a1);
        kb_store_pair(z0, a0, z1, a1, out, win, zh, at);
    });
}

// Cin = 3: thread = (output row, feature); the fmaf chain starts from w0 x0 (no bias: it cancels in the norm)
__global__ __launch_bounds__(KB_T) void kb_fwd3_kernel(const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss,
                                                       const float *__restrict__ w, const float *__restrict__ stats, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, int M, int dim, int F, float *__restrict__ out,
                                                       unsigned char *__restrict__ win, float *__restrict__ zh)
{
    const int64_t t = (int64_t)blockIdx.x * KB_T + threadIdx.x;
    if (t >= (int64_t)(M >> 1) * F) return;
    const int om = (int)(t / F), f = (int)(t - (int64_t)om * F);
    float z[2], a[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float *xr, *wr;
        const int o = kd_fwd3_row(2 * om + e, M, dim, sel, ss, x, ldx, w, f, xr, wr);
        const float acc = fmaf(wr[2], xr[2], fmaf(wr[1], xr[1], wr[0] * xr[0]));
        kb_affine(acc, kb_chan(stats, gamma, beta, 3 * F, o), z[e], a[e]);
    }
    kb_store_pair(z[0], a[0], z[1], a[1], out, win, zh, t);
}

// ---- backward: the sparse sums S, dbeta, dgamma ----------------------------------------------------------------------------------------
// chunk t (blockIdx.x) = rows 128 t .. + 127; wave = one 32 x 32 block (features 32 fb .. , input channels 32 cb ..) of each of the three
// planes (kd_dw_acc with two row sums).  part + t * pld: S [3F, Cin] of the chunk, then dbeta [3F], then dgamma [3F].
__global__ __launch_bounds__(KB_T) void kb_dw_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                     const float *__restrict__ zh, const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel,
                                                     int64_t ss, int M, int dim, int Cin, int F, float *__restrict__ part, int64_t pld)
{
    const int r = threadIdx.x & 31;
    const int ncb = Cin >> 5, id = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (id >= (F >> 5) * ncb) return;
    const int fb = id / ncb, cb = id - fb * ncb;
    floatx16 acc[3];
    float sums[2][3];                                              // dbeta, dgamma
    kd_dw_acc<2>(gout, outv, win, zh, x, ldx, sel, ss, M, dim, F, blockIdx.x * KD_CH, fb * 32 + r, cb * 32 + r, acc, sums);
    kd_dw_store<2>(acc, sums, part + (int64_t)blockIdx.x * pld, Cin, F, fb, cb);
}

// Cin = 3: chunk t = rows 256 t .. + 255; workgroup = 32 features (blockIdx.y) x 8 slices of the chunk's pooled rows (kd_dw3_chunk, 5 sums per plane)
__global__ __launch_bounds__(KB_T) void kb_dw3_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                      const float *__restrict__ zh, const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel,
                                                      int64_t ss, int M, int dim, int F, float *__restrict__ part, int64_t pld)
{
    __shared__ float red[8][15][32];
    kd_dw3_chunk<2>(gout, outv, win, zh, x, ldx, sel, ss, M, dim, F, blockIdx.x * (KD_CH3 / 2), blockIdx.y * 32, red, part + (int64_t)blockIdx.x * pld);
}

// thread = element (o, c) of dW; the c = 0 thread of a channel also writes dgamma, dbeta, the zero bias gradient and the coefficients
// coef = [r | r dbeta / M | r dgamma rstd / M] x [n_ch].  eval: the norm is a fixed affine map.
__global__ __launch_bounds__(KB_T) void kb_dwfin_kernel(const float *__restrict__ S, const float *__restrict__ dbg, const float *__restrict__ stats,
                                                        const float *__restrict__ gamma, const float *__restrict__ mean, const float *__restrict__ tm,
                                                        int M, int Cin, int n_ch, int eval, int accumulate, float *__restrict__ dw,
                                                        float *__restrict__ dbias, float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                        float *__restrict__ coef)
{
    const int64_t i = (int64_t)blockIdx.x * KB_T + threadIdx.x;
    if (i >= (int64_t)n_ch * Cin) return;
    const int o = (int)(i / Cin), c = (int)(i - (int64_t)o * Cin);
    const float rstd = stats[n_ch + o], r = gamma[o] * rstd, db = dbg[o], dg = dbg[n_ch + o];
    const float cg = eval ? 0.f : dg * rstd / (float)M;
    float g = S[i];
    if (!eval) g = g - db * mean[c] - cg * tm[i];
    g *= r;
    dw[i] = accumulate ? dw[i] + g : g;
    if (c != 0) return;
    dgamma[o] = accumulate ? dgamma[o] + dg : dg;
    dbeta[o] = accumulate ? dbeta[o] + db : db;
    if (dbias) {
        if (eval) dbias[o] = accumulate ? dbias[o] + r * db : r * db;
        else if (!accumulate) dbias[o] = 0.f;
    }
    coef[o] = r;
    coef[n_ch + o] = eval ? 0.f : r * db / (float)M;
    coef[2 * n_ch + o] = r * cg;
}

// ---- backward: A = W^T diag(e) W and v = W^T d ------------------------------------------------------------------------------------------
// wave = block (cb1, cb2) of A over the channels of slice blockIdx.y (ks_per k steps of 16 channels), in order: A-operand[row r = c1][o] =
// e_o W[o][32 cb1 + r], B[o][col r] = W[o][32 cb2 + r]; the cb1 = 0 waves also sum v[32 cb2 + r].  part + slice * (Cin^2 + Cin): [A | v].
__global__ __launch_bounds__(KB_T) void kb_a_kernel(const float *__restrict__ w, const float *__restrict__ coef, int Cin, int n_ch, int ks_per,
                                                    float *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int ncb = Cin >> 5, id = blockIdx.x * 4 + wv;
    if (id >= ncb * ncb) return;
    const int cb1 = id / ncb, cb2 = id - cb1 * ncb;
    const float *d = coef + n_ch, *e = coef + 2 * n_ch;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float vs = 0.f;
    const int o_lo = blockIdx.y * ks_per * 16, o_hi = min(o_lo + ks_per * 16, n_ch);
    for (int o0 = o_lo; o0 < o_hi; o0 += 16) {                     // (3F is a multiple of 32)
        float av[8], bv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int o = o0 + 8 * h + j;
            const float *wr = w + (int64_t)o * Cin;
            av[j] = e[o] * wr[cb1 * 32 + r];
            bv[j] = wr[cb2 * 32 + r];
            vs = fmaf(d[o], bv[j], vs);
        }
        acc = kd_step(av, bv, acc);
    }
    float *am = part + (int64_t)blockIdx.y * ((int64_t)Cin * Cin + Cin);
#pragma unroll
    for (int i = 0; i < 16; ++i) am[(int64_t)(cb1 * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * Cin + cb2 * 32 + r] = acc[i];
    const float tot = vs + __shfl_xor(vs, 32);
    if (cb1 == 0 && h == 0) am[(int64_t)Cin * Cin + cb2 * 32 + r] = tot;
}

// Cin = 3: thread t < 9 = element of A, t = 9 .. 11 = element of v
__global__ __launch_bounds__(64) void kb_a3_kernel(const float *__restrict__ w, const float *__restrict__ coef, int n_ch, float *__restrict__ am,
                                                   float *__restrict__ v)
{
    const int t = threadIdx.x;
    if (t >= 12) return;
    const float *d = coef + n_ch, *e = coef + 2 * n_ch;
    float s = 0.f;
    if (t < 9) {
        const int c1 = t / 3, c2 = t - 3 * c1;
        for (int o = 0; o < n_ch; ++o) s = fmaf(e[o] * w[3 * o + c1], w[3 * o + c2], s);
        am[t] = s;
    } else {
        for (int o = 0; o < n_ch; ++o) s = fmaf(d[o], w[3 * o + t - 9], s);
        v[t - 9] = s;
    }
}

// ---- backward: dX -------------------------------------------------------------------------------------------------------------------
// dy of a selected winner with out > 0: the pooled gradient times r_c (coef's first block), c = 3f + q
struct KbDyScaled {
    const float *r;
    __device__ __forceinline__ float operator()(float g, int c) const { return g * r[c]; }
};

// wave: source rows m0 .. m0 + 31 (blockIdx.x), input channels 32 cb .. + 31 (cb = 4 blockIdx.y + wave): kd_dx_acc with dy = r_c g; then the
// dense term in the same accumulator, A[row r][c] = x[m0 + r][c] - xm[c], B[c][col r] = -A[32 cb + r][c] (A's triangles agree to rounding),
// and v is subtracted in the epilogue.
__global__ __launch_bounds__(KB_T) void kb_dx_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                     const int *__restrict__ sel, int64_t ss, const float *__restrict__ w, const float *__restrict__ coef,
                                                     const float *__restrict__ x, int64_t ldx, const float *__restrict__ mean, const float *__restrict__ am,
                                                     const float *__restrict__ v, int dense, int M, int dim, int Cin, int F, float *__restrict__ dx,
                                                     int64_t ldd)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int cb = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (cb * 32 >= Cin) return;
    const int m0 = blockIdx.x * 32, m = m0 + r;
    const bool live = m < M;
    floatx16 acc = kd_dx_acc(gout, outv, win, sel, ss, w, M, dim, Cin, F, m0, cb, KbDyScaled{coef});
    float vc = 0.f;
    if (dense) {
        const float *xr = x + (int64_t)(live ? m : 0) * ldx + 8 * h, *ar = am + (int64_t)(cb * 32 + r) * Cin + 8 * h, *mr = mean + 8 * h;
        for (int c0 = 0; c0 < Cin; c0 += 16) {
            float av[8], bv[8], mv[8];
            kd_ld8(xr + c0, av);
            kd_ld8(mr + c0, mv);
            kd_ld8(ar + c0, bv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                av[j] = live ? av[j] - mv[j] : 0.f;
                bv[j] = -bv[j];
            }
            acc = kd_step(av, bv, acc);
        }
        vc = v[cb * 32 + r];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int mm = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (mm < M) dx[(int64_t)mm * ldd + cb * 32 + r] = acc[i] - vc;
    }
}

// Cin = 3: thread = source row
__global__ __launch_bounds__(KB_T) void kb_dx3_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                      const int *__restrict__ sel, int64_t ss, const float *__restrict__ w, const float *__restrict__ coef,
                                                      const float *__restrict__ x, int64_t ldx, const float *__restrict__ mean, const float *__restrict__ am,
                                                      const float *__restrict__ v, int dense, int M, int dim, int F, float *__restrict__ dx, int64_t ldd)
{
    const int m = blockIdx.x * KB_T + threadIdx.x;
    if (m >= M) return;
    float a[3] = {0.f, 0.f, 0.f};
    kd_dx3_acc(gout, outv, win, sel, ss, w, m, dim, F, a, KbDyScaled{coef});
    if (dense) {
        const float *xr = x + (int64_t)m * ldx;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t = xr[c] - mean[c];
            a[0] = fmaf(-t, am[3 * c], a[0]);
            a[1] = fmaf(-t, am[3 * c + 1], a[1]);
            a[2] = fmaf(-t, am[3 * c + 2], a[2]);
        }
        a[0] -= v[0]; a[1] -= v[1]; a[2] -= v[2];
    }
    float *o = dx + (int64_t)m * ldd;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
static size_t kb_pad4(size_t n) { return (n + 3) & ~(size_t)3; }             // floats: every block of a workspace stays 16-byte aligned
static int64_t kb_mchunks(int64_t M) { return cdiv(M, KB_MCH); }
// kb_a_kernel's slices of the 3F channels: about 2048 waves in all, at least 8 k steps each; 1 = written in place, no fold
static int kb_a_slices(int Cin, int F)
{
    if (Cin == 3) return 1;
    const int ncb = Cin / 32, ks = 3 * F / 16;
    return std::max(1, std::min(2048 / (ncb * ncb), ks / 8));
}

// workspace of the train-mode forward: [column-sum partials | second-moment partials | C]; the eval-mode forward takes none
struct KbFwdPtrs { float *psum, *pgram, *cm; };
static size_t kb_fwd_layout(int B, int dim, int Cin, bool training, void *base, KbFwdPtrs &p)
{
    WsCarver c{static_cast<char *>(base), 0, 16};
    const size_t T = (size_t)kb_mchunks((int64_t)B * dim), cc = (size_t)Cin * Cin;
    if (training) { p.psum = c.take<float>(T * Cin); p.pgram = c.take<float>(T * cc); p.cm = c.take<float>(kb_pad4(cc)); }
    return c.off;
}

// workspace of the backward: [chunk partials (S | dbeta | dgamma) | S | dbeta, dgamma | coefficients 3 x 3F | A | v | A, v per slice]
struct KbBwdPtrs { float *part, *S, *dbg, *coef, *am, *v, *apart; int64_t n1, n2; };
static size_t kb_bwd_layout(int B, int dim, int Cin, int F, void *base, KbBwdPtrs &p)
{
    WsCarver c{static_cast<char *>(base), 0, 16};
    const size_t T = (size_t)kd_level_chunks((int64_t)B * dim, Cin), S = (size_t)kb_a_slices(Cin, F);
    p.n1 = (int64_t)kb_pad4((size_t)3 * F * Cin); p.n2 = (int64_t)6 * F;
    p.part = c.take<float>(T * (size_t)(p.n1 + p.n2));
    p.S = c.take<float>((size_t)p.n1); p.dbg = c.take<float>((size_t)p.n2); p.coef = c.take<float>((size_t)9 * F);
    p.am = c.take<float>((size_t)Cin * Cin); p.v = c.take<float>(kb_pad4(Cin));
    p.apart = S > 1 ? c.take<float>(S * ((size_t)Cin * Cin + Cin)) : p.am;       // (slices only for Cin % 32 == 0: unpadded; one: A is written in place)
    return c.off;
}

}  // namespace papc

using namespace papc;

extern "C" {

int papc_kdbn_ok(int dim, int Cin, int F) { return kd_level_ok(dim, Cin, F, KB_FMAX) ? 1 : 0; }

size_t papc_kdbn_fwd_workspace(int B, int dim, int Cin, int F)
{
    if (B < 1 || !kd_level_ok(dim, Cin, F, KB_FMAX) || (int64_t)B * dim > ((int64_t)1 << 28)) return 0;
    KbFwdPtrs p;
    return kb_fwd_layout(B, dim, Cin, true, nullptr, p);
}

int papc_kdbn_fwd_f32(const float *x, int64_t ldx, const int32_t *sel, int64_t sel_stride, const float *w, const float *bias, const float *gamma,
                      const float *beta, float *running_mean, float *running_var, int B, int dim, int Cin, int F, float eps, float momentum, int training,
                      float *out, uint8_t *win, float *zhat, float *mean, float *tmat, float *stats, void *workspace, size_t workspace_bytes,
                      papc_stream_t stream)
{
    const char *who = "papc_kdbn_fwd_f32";
    PAPC_REQUIRE(x && sel && w && gamma && beta && out && win && zhat && stats, PAPC_E_INVALID, "%s: null pointer", who);
    int err = kd_level_shape_ok(who, B, dim, Cin, F, KB_FMAX);
    if (err != PAPC_OK) return err;
    err = kd_level_fwd_args_ok(who, x, ldx, sel_stride, w, dim, Cin);
    if (err != PAPC_OK) return err;
    hipStream_t st = as_stream(stream);
    const int M = B * dim, n_ch = 3 * F;
    KbFwdPtrs p;
    const size_t need = kb_fwd_layout(B, dim, Cin, training != 0, workspace, p);
    if (training) {
        PAPC_REQUIRE(mean && tmat && workspace, PAPC_E_INVALID, "%s: train mode needs mean, tmat and a workspace", who);
        PAPC_REQUIRE(workspace_bytes >= need && aligned16(workspace) && aligned16(mean) && aligned16(tmat), PAPC_E_INVALID,
                     "%s: workspace %zu bytes < %zu (or workspace / mean / tmat not 16-byte aligned)", who, workspace_bytes, need);
        const int T = (int)kb_mchunks(M);
        const size_t cc = (size_t)Cin * Cin;
        {
            ProfScope prof(PAPC_K_MISC, st);
            hipLaunchKernelGGL(kb_colsum_kernel, dim3((unsigned)T, (unsigned)cdiv(Cin, 16)), dim3(KB_T), 0, st, x, ldx, M, Cin, p.psum);
            hipLaunchKernelGGL(kb_mean_kernel, dim3((unsigned)cdiv(Cin, KB_T)), dim3(KB_T), 0, st, p.psum, T, M, Cin, mean);
            if (Cin == 3)
                hipLaunchKernelGGL(kb_gram3_kernel, dim3((unsigned)T), dim3(KB_T), 0, st, x, ldx, mean, M, p.pgram);
            else
                hipLaunchKernelGGL(kb_gram_kernel, dim3((unsigned)T, (unsigned)cdiv((int64_t)(Cin / 32) * (Cin / 32), 4)), dim3(KB_T), 0, st, x, ldx, mean, M,
                                   Cin, p.pgram);
            const int e = check_launch("papc_kdbn_fwd_f32: moments");
            if (e != PAPC_OK) return e;
        }
        int e = papc_reduce_partials_f32(p.pgram, T, (int64_t)cc, p.cm, 0, stream);      // the chunks in chunk order (fold.h)
        if (e != PAPC_OK) return e;
        ProfScope prof(PAPC_K_MISC, st);
        if (Cin == 3)
            hipLaunchKernelGGL(kb_t3_kernel, dim3((unsigned)cdiv(n_ch, KB_T)), dim3(KB_T), 0, st, w, p.cm, n_ch, tmat);
        else
            hipLaunchKernelGGL(kb_t_kernel, dim3((unsigned)(n_ch / 32), (unsigned)cdiv(Cin / 32, 4)), dim3(KB_T), 0, st, w, p.cm, Cin, tmat);
        hipLaunchKernelGGL(kb_finalize_kernel, dim3((unsigned)n_ch), dim3(64), 0, st, w, bias, mean, tmat, M, Cin, n_ch, eps, momentum, stats, running_mean,
                           running_var);
        e = check_launch("papc_kdbn_fwd_f32: statistics");
        if (e != PAPC_OK) return e;
    } else {
        PAPC_REQUIRE(running_mean && running_var, PAPC_E_INVALID, "%s: eval mode needs the running statistics", who);
        ProfScope prof(PAPC_K_MISC, st);
        hipLaunchKernelGGL(kb_eval_kernel, dim3((unsigned)cdiv(n_ch, KB_T)), dim3(KB_T), 0, st, bias, running_mean, running_var, n_ch, eps, stats);
    }
    ProfScope prof(PAPC_K_MLP_GEMM, st);
    if (Cin == 3)
        hipLaunchKernelGGL(kb_fwd3_kernel, dim3((unsigned)cdiv((int64_t)(M / 2) * F, KB_T)), dim3(KB_T), 0, st, x, ldx, sel, sel_stride, w, stats, gamma, beta, M,
                           dim, F, out, win, zhat);
    else
        hipLaunchKernelGGL(kb_fwd_kernel, dim3((unsigned)cdiv(M, 32), (unsigned)cdiv(F / 32, 4)), dim3(KB_T), 0, st, x, ldx, sel, sel_stride, w, stats, gamma,
                           beta, M, dim, Cin, F, out, win, zhat);
    return check_launch(who);
}

size_t papc_kdbn_bwd_workspace(int B, int dim, int Cin, int F)
{
    if (B < 1 || !kd_level_ok(dim, Cin, F, KB_FMAX) || (int64_t)B * dim > ((int64_t)1 << 28)) return 0;
    KbBwdPtrs p;
    return kb_bwd_layout(B, dim, Cin, F, nullptr, p);
}

int papc_kdbn_bwd_f32(const float *gout, const float *out, const uint8_t *win, const float *zhat, const float *x, int64_t ldx, const int32_t *sel,
                      int64_t sel_stride, const float *w, const float *gamma, const float *mean, const float *tmat, const float *stats, int B, int dim,
                      int Cin, int F, int training, float *dx, int64_t ldd, float *dw, float *dbias, float *dgamma, float *dbeta, int accumulate,
                      void *workspace, size_t workspace_bytes, papc_stream_t stream)
{
    const char *who = "papc_kdbn_bwd_f32";
    PAPC_REQUIRE(gout && out && win && zhat && x && sel && w && gamma && stats && dw && dgamma && dbeta && workspace, PAPC_E_INVALID, "%s: null pointer", who);
    int err = kd_level_shape_ok(who, B, dim, Cin, F, KB_FMAX);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(!training || (mean && tmat), PAPC_E_INVALID, "%s: train mode needs the forward's mean and tmat", who);
    KbBwdPtrs p;
    const size_t need = kb_bwd_layout(B, dim, Cin, F, workspace, p);
    // (the dense dX term reads x and mean by vector loads)
    err = kd_level_bwd_args_ok(who, gout, out, win, ldx, sel_stride, dx != nullptr, ldd, dim, Cin, aligned16(x) && ldx % 4 == 0 && (!training || aligned16(mean)),
                               "gout, out, x and mean must be 16-byte aligned, ldx a multiple of 4, the winner bytes 8-byte aligned", workspace, workspace_bytes, need);
    if (err != PAPC_OK) return err;
    hipStream_t st = as_stream(stream);
    const int M = B * dim, n_ch = 3 * F, T = (int)kd_level_chunks(M, Cin), dense = training ? 1 : 0;
    const int64_t n1 = p.n1, n2 = p.n2;
    {
        ProfScope prof(PAPC_K_BWD_DW, st);
        if (Cin == 3)
            hipLaunchKernelGGL(kb_dw3_kernel, dim3((unsigned)T, (unsigned)(F / 32)), dim3(KB_T), 0, st, gout, out, win, zhat, x, ldx, sel, sel_stride, M, dim, F,
                               p.part, n1 + n2);
        else
            hipLaunchKernelGGL(kb_dw_kernel, dim3((unsigned)T, (unsigned)cdiv((int64_t)(F / 32) * (Cin / 32), 4)), dim3(KB_T), 0, st, gout, out, win, zhat, x, ldx,
                               sel, sel_stride, M, dim, Cin, F, p.part, n1 + n2);
        const int e = check_launch("papc_kdbn_bwd_f32: S");
        if (e != PAPC_OK) return e;
    }
    // the chunks in chunk order (fold.h)
    int e = papc_reduce_partials2_f32(p.part, T, n1 + n2, n1, p.S, n2, p.dbg, 0, stream);
    if (e != PAPC_OK) return e;
    {
        ProfScope prof(PAPC_K_BWD_DW, st);
        hipLaunchKernelGGL(kb_dwfin_kernel, dim3((unsigned)cdiv((int64_t)n_ch * Cin, KB_T)), dim3(KB_T), 0, st, p.S, p.dbg, stats, gamma, mean, tmat, M, Cin, n_ch,
                           training ? 0 : 1, accumulate, dw, dbias, dgamma, dbeta, p.coef);
        e = check_launch("papc_kdbn_bwd_f32: dW");
        if (e != PAPC_OK) return e;
    }
    if (!dx) return PAPC_OK;
    if (dense) {
        int S = 1, ks_per = n_ch / 16;
        const int64_t na = (int64_t)Cin * Cin + Cin;                                           // (v follows A: a slice's layout)
        {
            ProfScope prof(PAPC_K_BWD_DX, st);
            if (Cin == 3)
                hipLaunchKernelGGL(kb_a3_kernel, dim3(1), dim3(64), 0, st, w, p.coef, n_ch, p.am, p.v);
            else {
                ks_per = (int)cdiv(n_ch / 16, kb_a_slices(Cin, F));
                S = (int)cdiv(n_ch / 16, ks_per);
                hipLaunchKernelGGL(kb_a_kernel, dim3((unsigned)cdiv((int64_t)(Cin / 32) * (Cin / 32), 4), (unsigned)S), dim3(KB_T), 0, st, w, p.coef, Cin, n_ch,
                                   ks_per, p.apart);
            }
            e = check_launch("papc_kdbn_bwd_f32: A");
            if (e != PAPC_OK) return e;
        }
        if (S > 1) {
            e = papc_reduce_partials_f32(p.apart, S, na, p.am, 0, stream);                     // the slices in slice order (fold.h)
            if (e != PAPC_OK) return e;
        }
    }
    ProfScope prof(PAPC_K_BWD_DX, st);
    if (Cin == 3)
        hipLaunchKernelGGL(kb_dx3_kernel, dim3((unsigned)cdiv(M, KB_T)), dim3(KB_T), 0, st, gout, out, win, sel, sel_stride, w, p.coef, x, ldx, mean, p.am, p.v, dense, M,
                           dim, F, dx, ldd);
    else
        hipLaunchKernelGGL(kb_dx_kernel, dim3((unsigned)cdiv(M, 32), (unsigned)cdiv(Cin / 32, 4)), dim3(KB_T), 0, st, gout, out, win, sel, sel_stride, w, p.coef, x,
                           ldx, mean, p.am, p.v, dense, M, dim, Cin, F, dx, ldd);
    return check_launch("papc_kdbn_bwd_f32: dX");
}

}  // extern "C"
