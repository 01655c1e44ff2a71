// kdconv.hip -- one level of the KD-Net classifier, for gfx950: 1x1 conv to 3F channels, ReLU, the kd-tree select, the max over point pairs.
//
// Reference: PAPC/models/classify/kdnet/kdnet.py:21-30
//     x = relu(conv(x));  x = reshape(x, (-1, F, 3, dim));  x = reshape(x, (-1, F, 3 * dim));
//     x = index_select(x, axis=2, index=sel + 3 * arange(dim));  x = max(reshape(x, (-1, F, dim / 2, 2)), axis=-1)
// The reshapes lay the selected axis out as k * dim + n (k = conv channel 3f + k, n = point) and the index is 3n + s, so for pre-pool
// row n of a cloud, s = sel[n] in {0, 1, 2}:
//     j = 3n + s    k = j / dim (weight plane)    p = j % dim (source point)
//     y[n, f] = relu(bias[3f + k] + sum_c W[3f + k, c] x[p, c])        out[m, f] = max(y[2m, f], y[2m + 1, f])
// (not the paper's "point n takes plane sel[n]": the source is reproduced as it is).  Only the selected third of the conv is
// computed, and the [rows, 3F] activations are never stored.  Rows are point-major: x [B * dim, Cin], out [B * dim / 2, F].
// The bodies of the kernels are kdlevel.h's, shared with kdbn.hip; this file adds the bias-and-ReLU epilogue, the Cin = 3 forward and the entry points.
//
//   forward   kd_fwd_kernel: a wave owns 32 consecutive rows of the flattened B * dim rows and 32 features (kd_fwd_acc); the pair max in registers.
//   backward  dy[n, f] = gout[n / 2, f] where row n won its pair and out > 0, else 0 (winner byte: 0 = the even row, also on an exact tie).
//             kd_dx_kernel: dX[p] = sum_q dy[n_q] . W_plane q over the rows that p feeds (kd_dx_acc); points that feed no row get exact zeros.
//             kd_dw_kernel: chunks of 128 rows; per chunk the partial dW [3F, Cin] (one accumulator per plane) and db [3F] (kd_dw_acc); folded in
//             chunk order by papc_reduce_partials2_f32 (fold.h).  No float atomics: two runs are bit-identical.
// Products: bf16x3.h on v_mfma_f32_32x32x16_bf16 (fp32 accuracy, fp32 accumulation).  The Cin = 3 first level runs fmaf chains on the vector
// unit (kd_fwd3_kernel, kd_dx3_kernel, kd_dw3_kernel).  Plain C++ loads and stores only.
#include "kdlevel.h"    // the index rule, the shared bodies of the kernels below and the host checks: shared with kdbn.hip

namespace papc {

constexpr int KD_FMAX = 512;     // the widest level

__device__ __forceinline__ void kd_store_pair(float y0, float y1, float *__restrict__ out, unsigned char *__restrict__ win, int64_t at)
{
    const bool w1 = y1 > y0 || (y1 != y1 && y0 == y0);     // the first row on an exact tie; a NaN goes through, as the source's max does
    out[at] = w1 ? y1 : y0;
    win[at] = w1 ? 1 : 0;
}

// plane k's of three values (by value: selects, where the same ternary on a lambda's captures compiles to branches)
__device__ __forceinline__ float kd_plane(int k, float v0, float v1, float v2) { return k == 0 ? v0 : (k == 1 ? v1 : v2); }

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// wave: rows m0 .. m0 + 31 (blockIdx.x), features 32 fb .. + 31 (fb = 4 blockIdx.y + wave): kd_fwd_acc, then per pair relu(acc + bias_k)
__global__ __launch_bounds__(KD_T) void kd_fwd_kernel(const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss,
                                                      const float *__restrict__ w, const float *__restrict__ bias, int M, int dim, int Cin, int F,
                                                      float *__restrict__ out, unsigned char *__restrict__ win)
{
    const int fb = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (fb * 32 >= F) return;
    const int m0 = blockIdx.x * 32, f = fb * 32 + (threadIdx.x & 31);
    int k;
    const floatx16 acc = kd_fwd_acc(x, ldx, sel, ss, w, M, dim, Cin, m0, f, k);
    const float bq0 = bias ? bias[3 * f] : 0.f, bq1 = bias ? bias[3 * f + 1] : 0.f, bq2 = bias ? bias[3 * f + 2] : 0.f;
    kd_fwd_pairs(acc, k, m0, M, F, f, [&](float acc0, int k0, float acc1, int k1, int64_t at) {
        kd_store_pair(relu_np(acc0 + kd_plane(k0, bq0, bq1, bq2)), relu_np(acc1 + kd_plane(k1, bq0, bq1, bq2)), out, win, at);
    });
}

// Cin = 3: thread = (output row, feature); the fmaf chain starts from the bias
__global__ __launch_bounds__(KD_T) void kd_fwd3_kernel(const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss,
                                                       const float *__restrict__ w, const float *__restrict__ bias, int M, int dim, int F,
                                                       float *__restrict__ out, unsigned char *__restrict__ win)
{
    const int64_t t = (int64_t)blockIdx.x * KD_T + threadIdx.x;
    if (t >= (int64_t)(M >> 1) * F) return;
    const int om = (int)(t / F), f = (int)(t - (int64_t)om * F);
    float y[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float *xr, *wr;
        const int o = kd_fwd3_row(2 * om + e, M, dim, sel, ss, x, ldx, w, f, xr, wr);
        float a = bias ? bias[o] : 0.f;
        a = fmaf(wr[0], xr[0], a);
        a = fmaf(wr[1], xr[1], a);
        a = fmaf(wr[2], xr[2], a);
        y[e] = relu_np(a);
    }
    kd_store_pair(y[0], y[1], out, win, t);
}

// ---- backward: dX -------------------------------------------------------------------------------------------------------------------
// wave: source rows m0 .. m0 + 31 (blockIdx.x), input channels 32 cb .. + 31 (cb = 4 blockIdx.y + wave): kd_dx_acc with dy = the pooled gradient
__global__ __launch_bounds__(KD_T) void kd_dx_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                     const int *__restrict__ sel, int64_t ss, const float *__restrict__ w, int M, int dim, int Cin, int F,
                                                     float *__restrict__ dx, int64_t ldd)
{
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int cb = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (cb * 32 >= Cin) return;
    const int m0 = blockIdx.x * 32;
    const floatx16 acc = kd_dx_acc(gout, outv, win, sel, ss, w, M, dim, Cin, F, m0, cb, KdDyPlain());
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int mm = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (mm < M) dx[(int64_t)mm * ldd + cb * 32 + r] = acc[i];
    }
}

// Cin = 3: thread = source row
__global__ __launch_bounds__(KD_T) void kd_dx3_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                      const int *__restrict__ sel, int64_t ss, const float *__restrict__ w, int M, int dim, int F,
                                                      float *__restrict__ dx, int64_t ldd)
{
    const int m = blockIdx.x * KD_T + threadIdx.x;
    if (m >= M) return;
    float a[3] = {0.f, 0.f, 0.f};
    kd_dx3_acc(gout, outv, win, sel, ss, w, m, dim, F, a, KdDyPlain());
    float *o = dx + (int64_t)m * ldd;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
}

// ---- backward: dW, db ---------------------------------------------------------------------------------------------------------------
// chunk t (blockIdx.x) = rows 128 t .. + 127; wave = one 32 x 32 block (features 32 fb .. , input channels 32 cb ..) of each of the three
// planes (kd_dw_acc with one row sum).  part + t * pld: dW [3F, Cin] of the chunk, then db [3F].
__global__ __launch_bounds__(KD_T) void kd_dw_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                     const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss, int M, int dim,
                                                     int Cin, int F, float *__restrict__ part, int64_t pld)
{
    const int r = threadIdx.x & 31;
    const int ncb = Cin >> 5, id = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (id >= (F >> 5) * ncb) return;
    const int fb = id / ncb, cb = id - fb * ncb;
    floatx16 acc[3];
    float dbs[1][3];
    kd_dw_acc<1>(gout, outv, win, nullptr, x, ldx, sel, ss, M, dim, F, blockIdx.x * KD_CH, fb * 32 + r, cb * 32 + r, acc, dbs);
    kd_dw_store<1>(acc, dbs, part + (int64_t)blockIdx.x * pld, Cin, F, fb, cb);
}

// Cin = 3: chunk t = rows 256 t .. + 255; workgroup = 32 features (blockIdx.y) x 8 slices of the chunk's pooled rows (kd_dw3_chunk, 4 sums per plane)
__global__ __launch_bounds__(KD_T) void kd_dw3_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                      const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss, int M, int dim,
                                                      int F, float *__restrict__ part, int64_t pld)
{
    __shared__ float red[8][12][32];
    kd_dw3_chunk<1>(gout, outv, win, nullptr, x, ldx, sel, ss, M, dim, F, blockIdx.x * (KD_CH3 / 2), blockIdx.y * 32, red, part + (int64_t)blockIdx.x * pld);
}

}  // namespace papc

using namespace papc;

extern "C" {

int papc_kdconv_ok(int dim, int Cin, int F) { return kd_level_ok(dim, Cin, F, KD_FMAX) ? 1 : 0; }

int papc_kdconv_fwd_f32(const float *x, int64_t ldx, const int32_t *sel, int64_t sel_stride, const float *w, const float *bias, int B, int dim, int Cin,
                        int F, float *out, uint8_t *win, papc_stream_t stream)
{
    const char *who = "papc_kdconv_fwd_f32";
    PAPC_REQUIRE(x && sel && w && out && win, PAPC_E_INVALID, "%s: null pointer", who);
    int err = kd_level_shape_ok(who, B, dim, Cin, F, KD_FMAX);
    if (err != PAPC_OK) return err;
    err = kd_level_fwd_args_ok(who, x, ldx, sel_stride, w, dim, Cin);
    if (err != PAPC_OK) return err;
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MLP_GEMM, st);
    const int M = B * dim;
    if (Cin == 3)
        hipLaunchKernelGGL(kd_fwd3_kernel, dim3((unsigned)cdiv((int64_t)(M / 2) * F, KD_T)), dim3(KD_T), 0, st, x, ldx, sel, sel_stride, w, bias, M, dim, F,
                           out, win);
    else
        hipLaunchKernelGGL(kd_fwd_kernel, dim3((unsigned)cdiv(M, 32), (unsigned)cdiv(F / 32, 4)), dim3(KD_T), 0, st, x, ldx, sel, sel_stride, w, bias, M, dim,
                           Cin, F, out, win);
    return check_launch(who);
}

size_t papc_kdconv_bwd_workspace(int B, int dim, int Cin, int F)
{
    if (B < 1 || !kd_level_ok(dim, Cin, F, KD_FMAX) || (int64_t)B * dim > ((int64_t)1 << 28)) return 0;
    return (size_t)kd_level_chunks((int64_t)B * dim, Cin) * ((size_t)3 * F * Cin + (size_t)3 * F) * sizeof(float);
}

int papc_kdconv_bwd_f32(const float *gout, const float *out, const uint8_t *win, const float *x, int64_t ldx, const int32_t *sel, int64_t sel_stride,
                        const float *w, int B, int dim, int Cin, int F, float *dx, int64_t ldd, float *dw, float *dbias, int accumulate, void *workspace,
                        size_t workspace_bytes, papc_stream_t stream)
{
    const char *who = "papc_kdconv_bwd_f32";
    PAPC_REQUIRE(gout && out && win && x && sel && w && dw && workspace, PAPC_E_INVALID, "%s: null pointer", who);
    int err = kd_level_shape_ok(who, B, dim, Cin, F, KD_FMAX);
    if (err != PAPC_OK) return err;
    err = kd_level_bwd_args_ok(who, gout, out, win, ldx, sel_stride, dx != nullptr, ldd, dim, Cin, true,
                               "gout and out must be 16-byte aligned, the winner bytes 8-byte aligned", workspace, workspace_bytes,
                               papc_kdconv_bwd_workspace(B, dim, Cin, F));
    if (err != PAPC_OK) return err;
    hipStream_t st = as_stream(stream);
    const int M = B * dim;
    if (dx) {
        ProfScope prof(PAPC_K_BWD_DX, st);
        if (Cin == 3)
            hipLaunchKernelGGL(kd_dx3_kernel, dim3((unsigned)cdiv(M, KD_T)), dim3(KD_T), 0, st, gout, out, win, sel, sel_stride, w, M, dim, F, dx, ldd);
        else
            hipLaunchKernelGGL(kd_dx_kernel, dim3((unsigned)cdiv(M, 32), (unsigned)cdiv(Cin / 32, 4)), dim3(KD_T), 0, st, gout, out, win, sel, sel_stride, w, M,
                               dim, Cin, F, dx, ldd);
        const int e = check_launch("papc_kdconv_bwd_f32: dX");
        if (e != PAPC_OK) return e;
    }
    const int T = (int)kd_level_chunks(M, Cin);
    const int64_t n1 = (int64_t)3 * F * Cin, n2 = (int64_t)3 * F;
    float *part = static_cast<float *>(workspace);
    {
        ProfScope prof(PAPC_K_BWD_DW, st);
        if (Cin == 3)
            hipLaunchKernelGGL(kd_dw3_kernel, dim3((unsigned)T, (unsigned)(F / 32)), dim3(KD_T), 0, st, gout, out, win, x, ldx, sel, sel_stride, M, dim, F, part,
                               n1 + n2);
        else
            hipLaunchKernelGGL(kd_dw_kernel, dim3((unsigned)T, (unsigned)cdiv((int64_t)(F / 32) * (Cin / 32), 4)), dim3(KD_T), 0, st, gout, out, win, x, ldx, sel,
                               sel_stride, M, dim, Cin, F, part, n1 + n2);
        const int e = check_launch("papc_kdconv_bwd_f32: dW");
        if (e != PAPC_OK) return e;
    }
    // the chunks in chunk order (fold.h); the bias gradient rides along when asked for
    return papc_reduce_partials2_f32(part, T, n1 + n2, n1, dw, dbias ? n2 : 0, dbias, accumulate, stream);
}

}  // extern "C"
