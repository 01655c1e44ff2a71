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
//
//   forward   kd_fwd_kernel: a wave owns 32 consecutive rows of the flattened B * dim rows and 32 features.  The points lie on the 32x32
//             accumulator's ROW axis (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so both rows of a pair are registers of one lane and the
//             pool needs no shuffle.  The wave loops over the planes present in its tile (a ballot); rows of another plane enter as zero A
//             rows, so a row's accumulator receives its own plane's products and exact zeros.  Operands straight from global memory.
//   backward  dy[n, f] = gout[n / 2, f] where row n won its pair and out > 0, else 0 (winner byte: 0 = the even row, also on an exact tie).
//             kd_dx_kernel: source point p feeds the rows with 3n + s = p + q dim, q = 0, 1, 2 (plane q) -- at most one row per q;
//             dX[p] = sum_q dy[n_q] . W_plane q, accumulated in that order; points that feed no row get exact zeros.
//             kd_dw_kernel: chunks of 128 rows; per chunk the partial dW [3F, Cin] (one accumulator per plane) and db [3F]; folded in
//             chunk order by papc_reduce_partials2_f32 (fold.h).  No float atomics: two runs are bit-identical.
// Products: bf16x3.h on v_mfma_f32_32x32x16_bf16 (fp32 accuracy, fp32 accumulation).  The Cin = 3 first level runs fmaf chains on the vector
// unit (kd_fwd3_kernel, kd_dx3_kernel, kd_dw3_kernel).  Plain C++ loads and stores only.
#include "bf16x3.h"
#include "kdsel.h"      // the select's index rule (kd_row_info, kd_fed_row), shared with kdbn.hip

namespace papc {

constexpr int KD_T = 256;        // threads of every kernel here (4 waves)
constexpr int KD_CH = 128;       // rows per dW chunk (MFMA kernel)
constexpr int KD_CH3 = 256;      // rows per dW chunk (Cin = 3 kernel)

__device__ __forceinline__ void kd_store_pair(float y0, float y1, float *__restrict__ out, unsigned char *__restrict__ win, int64_t at)
{
    const bool w1 = y1 > y0 || (y1 != y1 && y0 == y0);     // the first row on an exact tie; a NaN goes through, as the source's max does
    out[at] = w1 ? y1 : y0;
    win[at] = w1 ? 1 : 0;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// wave: rows m0 .. m0 + 31 (blockIdx.x), features 32 fb .. + 31 (fb = 4 blockIdx.y + wave).  A[row r][c] = x[source row of r][c] where r is
// of the plane at hand, B[c][col r] = W[3 (32 fb + r) + q][c]: both are 8 consecutive floats per lane and 16-wide k step.
__global__ __launch_bounds__(KD_T) void kd_fwd_kernel(const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss,
                                                      const float *__restrict__ w, const float *__restrict__ bias, int M, int dim, int Cin, int F,
                                                      float *__restrict__ out, unsigned char *__restrict__ win)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int fb = blockIdx.y * 4 + wv;
    if (fb * 32 >= F) return;
    const int m0 = blockIdx.x * 32;
    const unsigned info = kd_row_info(m0 + r, M, dim, sel, ss);
    const int k = (int)(info >> 30);
    const float *xr = x + (int64_t)(info & KD_ROW) * ldx + 8 * h;
    const int f = fb * 32 + r;
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
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 a0 = mine ? kd_ld4(xr + c0) : z, a1 = mine ? kd_ld4(xr + c0 + 4) : z;
            const float4 b0 = kd_ld4(wr + c0), b1 = kd_ld4(wr + c0 + 4);
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            bf16x8 ap[3], bp[3];
            split8(av, ap);
            split8(bv, bp);
            acc = mfma_bf16x3(ap, bp, acc);
        }
    }
    const float bq0 = bias ? bias[3 * f] : 0.f, bq1 = bias ? bias[3 * f + 1] : 0.f, bq2 = bias ? bias[3 * f + 2] : 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int row = 8 * g + 4 * h + 2 * t;      // lanes 0..31 hold the planes of rows 0..31
            const int k0 = __shfl(k, row), k1 = __shfl(k, row + 1);
            const int m = m0 + row;
            if (m < M) {                                // (M is even: row m + 1 exists)
                const float y0 = relu_np(acc[4 * g + 2 * t] + (k0 == 0 ? bq0 : (k0 == 1 ? bq1 : bq2)));
                const float y1 = relu_np(acc[4 * g + 2 * t + 1] + (k1 == 0 ? bq0 : (k1 == 1 ? bq1 : bq2)));
                kd_store_pair(y0, y1, out, win, (int64_t)(m >> 1) * F + f);
            }
        }
}

// Cin = 3: thread = (output row, feature)
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
        const unsigned info = kd_row_info(2 * om + e, M, dim, sel, ss);
        const float *xr = x + (int64_t)(info & KD_ROW) * ldx;
        const int o = 3 * f + (int)(info >> 30);
        const float *wr = w + (int64_t)o * 3;
        float a = bias ? bias[o] : 0.f;
        a = fmaf(wr[0], xr[0], a);
        a = fmaf(wr[1], xr[1], a);
        a = fmaf(wr[2], xr[2], a);
        y[e] = relu_np(a);
    }
    kd_store_pair(y[0], y[1], out, win, t);
}

// ---- backward: dX -------------------------------------------------------------------------------------------------------------------
// wave: source rows m0 .. m0 + 31, input channels 32 cb .. + 31.  A[row r][f] = dy[row fed by r through plane q][f] (8 consecutive f of
// one pooled row: gout, out and the winner bytes), B[f][col r] = W[3f + q][32 cb + r].
__global__ __launch_bounds__(KD_T) void kd_dx_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                     const int *__restrict__ sel, int64_t ss, const float *__restrict__ w, int M, int dim, int Cin, int F,
                                                     float *__restrict__ dx, int64_t ldd)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int cb = blockIdx.y * 4 + wv;
    if (cb * 32 >= Cin) return;
    const int m0 = blockIdx.x * 32, m = m0 + r;
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
                const float4 g0 = kd_ld4(gout + at + f0), g1 = kd_ld4(gout + at + f0 + 4), o0 = kd_ld4(outv + at + f0), o1 = kd_ld4(outv + at + f0 + 4);
                const uint2 wb = *reinterpret_cast<const uint2 *>(win + at + f0);
                const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, o[8] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned wj = ((j < 4 ? wb.x : wb.y) >> (8 * (j & 3))) & 0xffu;
                    av[j] = (o[j] > 0.f && wj == par) ? g[j] : 0.f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) av[j] = 0.f;
            }
            bf16x8 ap[3], bp[3];
            split8(av, ap);
            split8(bv, bp);
            acc = mfma_bf16x3(ap, bp, acc);
        }
    }
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
    const int b = m / dim, p = m - b * dim;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int q = 0; q < 3; ++q) {
        int n;
        if (!kd_fed_row(b, p, q, dim, sel, ss, n)) continue;
        const int64_t at = (((int64_t)b * dim + n) >> 1) * F;
        const unsigned par = (unsigned)(n & 1);
        for (int f = 0; f < F; ++f) {
            const float d = (outv[at + f] > 0.f && win[at + f] == par) ? gout[at + f] : 0.f;
            const float *wr = w + (int64_t)(3 * f + q) * 3;
            a0 = fmaf(d, wr[0], a0);
            a1 = fmaf(d, wr[1], a1);
            a2 = fmaf(d, wr[2], a2);
        }
    }
    float *o = dx + (int64_t)m * ldd;
    o[0] = a0; o[1] = a1; o[2] = a2;
}

// ---- backward: dW, db ---------------------------------------------------------------------------------------------------------------
// chunk t (blockIdx.x) = rows 128 t .. + 127; wave = one 32 x 32 block (features 32 fb .. , input channels 32 cb ..) of each of the three
// planes.  A[row r = feature][n] = dy[n][32 fb + r] for the rows n of plane q, B[n][col r] = x[source row of n][32 cb + r].
// part + t * pld: dW [3F, Cin] of the chunk, then db [3F].
__global__ __launch_bounds__(KD_T) void kd_dw_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                     const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss, int M, int dim,
                                                     int Cin, int F, float *__restrict__ part, int64_t pld)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int ncb = Cin >> 5, id = blockIdx.y * 4 + wv;
    if (id >= (F >> 5) * ncb) return;
    const int fb = id / ncb, cb = id - fb * ncb;
    const int f = fb * 32 + r;
    const int r0 = blockIdx.x * KD_CH;
    floatx16 acc[3];
    float dbs[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
    for (int ks = 0; ks < KD_CH / 16; ++ks) {
        const int mb = r0 + ks * 16;
        if (mb >= M) break;                                        // (wave-uniform)
        const unsigned info = kd_row_info(mb + (lane & 15), M, dim, sel, ss);     // the 16 rows of this k step, four times over
        const int kl = (int)(info >> 30);
        float dyv[8], bv[8];
        int kj[8];
#pragma unroll
        for (int t = 0; t < 4; ++t) {                              // rows mb + 8h + 2t, + 1 = pooled row (mb + 8h) / 2 + t
            const int mr = mb + 8 * h + 2 * t;
            float g = 0.f;
            unsigned wb = 0;
            if (mr < M) {
                const int64_t at = (int64_t)(mr >> 1) * F + f;
                g = outv[at] > 0.f ? gout[at] : 0.f;
                wb = win[at];
            }
            dyv[2 * t] = wb == 0 ? g : 0.f;
            dyv[2 * t + 1] = wb == 0 ? 0.f : g;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned inf = (unsigned)__shfl((int)info, 8 * h + j);
            kj[j] = (int)(inf >> 30);
            bv[j] = kj[j] < 3 ? x[(int64_t)(inf & KD_ROW) * ldx + cb * 32 + r] : 0.f;
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
            for (int j = 0; j < 8; ++j) dbs[q] += am[j];
            bf16x8 ap[3];
            split8(am, ap);
            acc[q] = mfma_bf16x3(ap, bp, acc[q]);
        }
    }
    float *pt = part + (int64_t)blockIdx.x * pld;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int fr = fb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            pt[(int64_t)(3 * fr + q) * Cin + cb * 32 + r] = acc[q][i];
        }
        const float tot = dbs[q] + __shfl_xor(dbs[q], 32);        // the two row halves of the lane pair
        if (cb == 0 && h == 0) pt[(int64_t)3 * F * Cin + 3 * f + q] = tot;
    }
}

// Cin = 3: chunk t = rows 256 t .. + 255; workgroup = 32 features (blockIdx.y) x 8 slices of the chunk's pooled rows.  Only the winner of a
// pair carries a gradient.  The slices are added in slice order.
__global__ __launch_bounds__(KD_T) void kd_dw3_kernel(const float *__restrict__ gout, const float *__restrict__ outv, const unsigned char *__restrict__ win,
                                                      const float *__restrict__ x, int64_t ldx, const int *__restrict__ sel, int64_t ss, int M, int dim,
                                                      int F, float *__restrict__ part, int64_t pld)
{
    __shared__ float red[8][12][32];
    const int fl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int f = blockIdx.y * 32 + fl;
    const int om0 = blockIdx.x * (KD_CH3 / 2);
    float a[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) a[i] = 0.f;
    for (int i = sl; i < KD_CH3 / 2; i += 8) {
        const int om = om0 + i;
        if (2 * om >= M) break;
        const int64_t at = (int64_t)om * F + f;
        const float g = outv[at] > 0.f ? gout[at] : 0.f;
        const unsigned info = kd_row_info(2 * om + (win[at] ? 1 : 0), M, dim, sel, ss);
        const int k = (int)(info >> 30);
        const float *xr = x + (int64_t)(info & KD_ROW) * ldx;
        const float x0 = xr[0], x1 = xr[1], x2 = xr[2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float d = k == q ? g : 0.f;
            a[4 * q] = fmaf(d, x0, a[4 * q]);
            a[4 * q + 1] = fmaf(d, x1, a[4 * q + 1]);
            a[4 * q + 2] = fmaf(d, x2, a[4 * q + 2]);
            a[4 * q + 3] += d;
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) red[sl][i][fl] = a[i];
    __syncthreads();
    if (sl != 0) return;
    float *pt = part + (int64_t)blockIdx.x * pld;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        float s = a[i];
#pragma unroll
        for (int g = 1; g < 8; ++g) s += red[g][i][fl];
        const int q = i >> 2, c = i & 3;
        if (c < 3) pt[(int64_t)(3 * f + q) * 3 + c] = s;
        else pt[(int64_t)3 * F * 3 + 3 * f + q] = s;
    }
}

static bool kd_ok(int dim, int Cin, int F)
{
    return dim >= 2 && dim % 2 == 0 && (Cin == 3 || (Cin >= 32 && Cin <= 512 && Cin % 32 == 0)) && F >= 32 && F <= 512 && F % 32 == 0;
}

static int kd_shape_ok(const char *who, int B, int dim, int Cin, int F)
{
    PAPC_REQUIRE(dim >= 2 && dim % 2 == 0, PAPC_E_UNSUPPORTED, "%s: dim=%d (points per cloud: even, >= 2)", who, dim);
    PAPC_REQUIRE(Cin == 3 || (Cin >= 32 && Cin <= 512 && Cin % 32 == 0), PAPC_E_UNSUPPORTED, "%s: Cin=%d (3, or a multiple of 32 up to 512)", who, Cin);
    PAPC_REQUIRE(F >= 32 && F <= 512 && F % 32 == 0, PAPC_E_UNSUPPORTED, "%s: F=%d (a multiple of 32 up to 512)", who, F);
    PAPC_REQUIRE(B >= 1 && (int64_t)B * dim <= ((int64_t)1 << 28), PAPC_E_INVALID, "%s: B=%d dim=%d (B >= 1, B * dim <= 2^28)", who, B, dim);
    return PAPC_OK;
}

static int64_t kd_chunks(int64_t M, int Cin) { return cdiv(M, Cin == 3 ? KD_CH3 : KD_CH); }

}  // namespace papc

using namespace papc;

extern "C" {

int papc_kdconv_ok(int dim, int Cin, int F) { return kd_ok(dim, Cin, F) ? 1 : 0; }

int papc_kdconv_fwd_f32(const float *x, int64_t ldx, const int32_t *sel, int64_t sel_stride, const float *w, const float *bias, int B, int dim, int Cin,
                        int F, float *out, uint8_t *win, papc_stream_t stream)
{
    PAPC_REQUIRE(x && sel && w && out && win, PAPC_E_INVALID, "papc_kdconv_fwd_f32: null pointer");
    const int err = kd_shape_ok("papc_kdconv_fwd_f32", B, dim, Cin, F);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(ldx >= Cin && (sel_stride == 0 || sel_stride >= dim), PAPC_E_INVALID, "papc_kdconv_fwd_f32: ldx=%lld < Cin or sel_stride=%lld (0 or >= dim)",
                 (long long)ldx, (long long)sel_stride);
    PAPC_REQUIRE(Cin == 3 || (ldx % 4 == 0 && aligned16(x) && aligned16(w)), PAPC_E_INVALID,
                 "papc_kdconv_fwd_f32: x and w must be 16-byte aligned, ldx=%lld a multiple of 4", (long long)ldx);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MLP_GEMM, st);
    const int M = B * dim;
    if (Cin == 3)
        hipLaunchKernelGGL(kd_fwd3_kernel, dim3((unsigned)cdiv((int64_t)(M / 2) * F, KD_T)), dim3(KD_T), 0, st, x, ldx, sel, sel_stride, w, bias, M, dim, F,
                           out, win);
    else
        hipLaunchKernelGGL(kd_fwd_kernel, dim3((unsigned)cdiv(M, 32), (unsigned)cdiv(F / 32, 4)), dim3(KD_T), 0, st, x, ldx, sel, sel_stride, w, bias, M, dim,
                           Cin, F, out, win);
    return check_launch("papc_kdconv_fwd_f32");
}

size_t papc_kdconv_bwd_workspace(int B, int dim, int Cin, int F)
{
    if (B < 1 || !kd_ok(dim, Cin, F) || (int64_t)B * dim > ((int64_t)1 << 28)) return 0;
    return (size_t)kd_chunks((int64_t)B * dim, Cin) * ((size_t)3 * F * Cin + (size_t)3 * F) * sizeof(float);
}

int papc_kdconv_bwd_f32(const float *gout, const float *out, const uint8_t *win, const float *x, int64_t ldx, const int32_t *sel, int64_t sel_stride,
                        const float *w, int B, int dim, int Cin, int F, float *dx, int64_t ldd, float *dw, float *dbias, int accumulate, void *workspace,
                        size_t workspace_bytes, papc_stream_t stream)
{
    PAPC_REQUIRE(gout && out && win && x && sel && w && dw && workspace, PAPC_E_INVALID, "papc_kdconv_bwd_f32: null pointer");
    const int err = kd_shape_ok("papc_kdconv_bwd_f32", B, dim, Cin, F);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(ldx >= Cin && (sel_stride == 0 || sel_stride >= dim) && (!dx || ldd >= Cin), PAPC_E_INVALID,
                 "papc_kdconv_bwd_f32: ldx=%lld < Cin, ldd=%lld < Cin or sel_stride=%lld (0 or >= dim)", (long long)ldx, (long long)ldd, (long long)sel_stride);
    PAPC_REQUIRE(Cin == 3 || (aligned16(gout) && aligned16(out) && (reinterpret_cast<uintptr_t>(win) & 7) == 0), PAPC_E_INVALID,
                 "papc_kdconv_bwd_f32: gout and out must be 16-byte aligned, the winner bytes 8-byte aligned");
    const size_t need = papc_kdconv_bwd_workspace(B, dim, Cin, F);
    PAPC_REQUIRE(workspace_bytes >= need && aligned16(workspace), PAPC_E_INVALID, "papc_kdconv_bwd_f32: workspace %zu bytes < %zu (or not 16-byte aligned)",
                 workspace_bytes, need);
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
    const int T = (int)kd_chunks(M, Cin);
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
