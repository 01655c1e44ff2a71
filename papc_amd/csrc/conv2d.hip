// conv2d.hip -- the PointPillars RPN's dense 2-D convolutions as implicit GEMMs, for gfx950: the 3x3 family (stride 1 or 2, zero halo 1) and the
// kernel = stride deconvolutions, forward, dX and dW, with the BatchNorm + ReLU of the producer applied on load.
//
// Reference: PAPC/models/detect/pointpillars/models/bones/rpn.py:71-133
//     Pad2D(1) + Conv2D(3, stride s) | Conv2D(3, padding=1), each + BatchNorm2D(eps 1e-3, momentum 0.01) + ReLU; Conv2DTranspose(kernel = stride)
//
// Layout: activations are channel-last rows [B H W, C] holding the PRE-norm conv output y (row = (b H + h) W + w); a consumer forms
// relu(scale y + shift) on load.  The weights keep the source's shapes ([Co, Ci, 3, 3], deconv [Ci, Co, s, s]); c2d_prep_kernel writes, once per
// step and for every layer in one launch, the two K-major orders the kernels read:
//     conv     wk [co][tap Ci + ci]        wt [ci][tap Co + co]         tap = 3 ty + tx
//     deconv   wk [ij][co][ci]             wt [ci][ij Co + co]          ij = s i + j
// The K order of every product is tap-major, k = tap * C + c.
//
// Every MFMA kernel is a wave per 32 x 32 output block of v_mfma_f32_32x32x16_bf16 through bf16x3.h (fp32 accuracy, fp32 accumulation), with the
// lane layout of voxconv.hip: lane (r = lane & 31, h = lane >> 5) holds A[row r][k = 8h + j] and B[k = 8h + j][col r], accumulator register i is row
// (i & 3) + 8 (i >> 2) + 4h of column r.  The operands are gathered from global memory by the im2col addressing (a pixel's channels are contiguous:
// two 16-byte loads per lane and k step).
//
//   c2d_fwd_kernel<NORM, DECONV, NT>   a wave owns 32 rows x NT column blocks (NT = 2 where the width is a multiple of 64): the A fragment is formed
//                         and split once per k step; the channel block is the outer loop, the taps the inner.  rows = output pixels (deconv: input pixels, blockIdx.z = the sub-position ij, the epilogue scatters to pixel
//                         (s h + i, s w + j) of a buffer with a leading dimension and a column offset).  A = plain rows or relu(scale y_prev + shift);
//                         the halo is selected to the exact 0 AFTER the norm.  Epilogue: y, and sum y / sum y^2 per channel, one partial row
//                         [2][Cout] per workgroup (128 rows; deconv: per workgroup and sub-position) -- the layout papc_bn_finalize_f32 folds.
//   c2d_dx_kernel<DECONV, NT>  rows = input pixels, NT column blocks per wave as above: dA[b, p, ci] = sum_tap sum_co dY[b, (p + 1 - tap) / s, co] W[co, ci, tap]; under stride 2 the
//                         taps of the wrong parity are selected away.  dY = scale (dz - c1 - xhat c2) on load from the stored dz, y and the
//                         layer's constants.  Epilogue: + the optional addend (the other consumer's dA), x ReLU' (sign of scale y_prev + shift,
//                         recomputed) -> dz_prev, and sum dz / sum dz xhat per workgroup -- the layout papc_bn_bwd_finalize_f32 folds.  Without a
//                         norm above (the canvas) the sum is stored as it is.
//   c2d_dw_kernel<NORM, DECONV>   dW[co, ci, tap] = sum_rows dY[row, co] a[src(row, tap), ci]: wave = tap, blockIdx.x = row chunk, blockIdx.y =
//                         the (co, ci) block.  Partials per chunk in the source's order, folded in chunk order (papc_reduce_partials_f32).
//   c2d_relu_bwd_kernel   the concat buffer's backward entry: dz = gout [scale y + shift > 0] and the two sums, per 64-row workgroup.
// No float atomics, every cross-workgroup sum a fixed-order fold: two runs are bit-identical.  Plain C++ loads and stores only.  Every k loop is
// straight-line -- an operand is always loaded, from an address that exists, and then selected -- and the accumulator is drained in front of each
// epilogue.
#include "bf16x3.h"

namespace papc {

constexpr int C2_T = 256;          // threads of every MFMA kernel here (4 waves)
constexpr int C2_CMAX = 256;       // widest layer
constexpr int C2_PREP_MAX = 32;    // layers per prep launch
constexpr int C2_DW_CHUNKS = 64;   // dW row chunks aimed at
constexpr int C2_RB_ROWS = 64;     // rows per workgroup of c2d_relu_bwd_kernel

// in side: B H W pixels of Cin channels; out side: B Ho Wo pixels of Cout channels.  conv: Ho = (H - 1) / s + 1; deconv: Ho = s H
struct C2Geo { int B, H, W, Ho, Wo, s, Cin, Cout; };

struct C2Norm { const float *mean, *invstd, *scale, *c1, *c2; };        // a layer's constants as its backward reads them
struct C2Prev { const float *y, *mean, *invstd, *scale, *shift; };      // the producer under a dX epilogue (y == nullptr: none)

struct C2PrepJobs {
    const float *w[C2_PREP_MAX];
    float *wk[C2_PREP_MAX], *wt[C2_PREP_MAX];
    int cin[C2_PREP_MAX], cout[C2_PREP_MAX], taps[C2_PREP_MAX], deconv[C2_PREP_MAX];
};

__device__ __forceinline__ floatx16 c2d_step(const float (&av)[8], const float (&bv)[8], floatx16 acc)
{
    bf16x8 ap[3], bp[3];
    split8(av, ap);
    split8(bv, bp);
    return mfma_bf16x3(ap, bp, acc);
}

__device__ __forceinline__ void c2d_ld8(const float *p, float (&v)[8])
{
    const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// behind a k loop, in front of the epilogue's first read of the accumulator (voxconv.hip::vox_mfma_drain)
__device__ __forceinline__ void c2d_mfma_drain(floatx16 &acc)
{
    asm volatile("s_nop 15" : "+a"(acc));
}

// the per-channel sums (s, q) of a workgroup's four waves -> dst[0][n0 + c], dst[1][n0 + c] of a [2][C] partial row
__device__ __forceinline__ void c2d_block_sums(float s, float q, float *__restrict__ dst, int C, int n0)
{
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    s += __shfl_xor(s, 32);
    q += __shfl_xor(q, 32);
    __syncthreads();                                                 // (a kernel calls this once per column block: the previous call's readers are done)
    if (lane < 32) { red[wv][lane] = s; red[wv][32 + lane] = q; }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int t = threadIdx.x;
        dst[(t >> 5) * C + n0 + (t & 31)] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
}

// ---- the K-major weight orders ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(C2_T) void c2d_prep_kernel(C2PrepJobs jb)
{
    const int l = blockIdx.y;
    const int cin = jb.cin[l], cout = jb.cout[l], taps = jb.taps[l];
    const int i = blockIdx.x * C2_T + threadIdx.x;
    if (i >= cin * cout * taps) return;
    const float v = jb.w[l][i];
    const int tap = i % taps, rem = i / taps;
    if (jb.deconv[l]) {                                             // [ci][co][ij]
        const int co = rem % cout, ci = rem / cout;
        jb.wk[l][((int64_t)tap * cout + co) * cin + ci] = v;
        jb.wt[l][((int64_t)ci * taps + tap) * cout + co] = v;
    } else {                                                        // [co][ci][tap]
        const int ci = rem % cin, co = rem / cin;
        jb.wk[l][((int64_t)co * taps + tap) * cin + ci] = v;
        jb.wt[l][((int64_t)ci * taps + tap) * cout + co] = v;
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------------
// A wave owns 32 rows x NT column blocks of 32: the A fragment is loaded, normed and split once per k step and meets NT B fragments.  The channel
// block is the outer loop, so its scale / shift are loaded once for the nine taps.
template <bool NORM, bool DECONV, int NT>
__global__ __launch_bounds__(C2_T) void c2d_fwd_kernel(const float *__restrict__ x, const float *__restrict__ sc_in, const float *__restrict__ sh_in,
                                                      const float *__restrict__ wk, C2Geo g, float *__restrict__ y, int ldy, int coff,
                                                      float *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int RH = DECONV ? g.H : g.Ho, RW = DECONV ? g.W : g.Wo, M = g.B * RH * RW;
    const int m0 = (blockIdx.x * 4 + wv) * 32, m = m0 + r, n0 = blockIdx.y * (32 * NT), z = blockIdx.z;
    const bool live = m < M;
    const int mc = live ? m : 0;
    const int b = mc / (RH * RW), p = mc - b * (RH * RW), ph = p / RW, pw = p - ph * RW;
    constexpr int taps = DECONV ? 1 : 9;
    const float *wr = wk + ((int64_t)(z * g.Cout + n0 + r) * taps) * g.Cin + 8 * h;
    const int64_t wstep = (int64_t)32 * taps * g.Cin;                                      // to the next column block
    floatx16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    for (int c = 0; c < g.Cin; c += 16) {
        float sc[8], sh[8];
        if (NORM) {
            c2d_ld8(sc_in + c + 8 * h, sc);
            c2d_ld8(sh_in + c + 8 * h, sh);
        }
#pragma unroll
        for (int tap = 0; tap < taps; ++tap) {
            const int ty = tap / 3, tx = tap - 3 * ty;
            const int hi = DECONV ? ph : ph * g.s + ty - 1, wi = DECONV ? pw : pw * g.s + tx - 1;
            const bool valid = live && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;        // else: the zero halo
            const int src = valid ? (b * g.H + hi) * g.W + wi : 0;                         // (the halo reads pixel 0 and selects nothing)
            float av[8];
            c2d_ld8(x + (int64_t)src * g.Cin + 8 * h + c, av);
            if (NORM) {
#pragma unroll
                for (int j = 0; j < 8; ++j) av[j] = relu_np(fmaf(sc[j], av[j], sh[j]));
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) av[j] = valid ? av[j] : 0.f;                       // the zero of the ACTIVATED tensor
            bf16x8 ap[3];
            split8(av, ap);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float bv[8];
                bf16x8 bp[3];
                c2d_ld8(wr + t * wstep + tap * g.Cin + c, bv);
                split8(bv, bp);
                acc[t] = mfma_bf16x3(ap, bp, acc[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) c2d_mfma_drain(acc[t]);
    const int zi = DECONV ? z / g.s : 0, zj = DECONV ? z - zi * g.s : 0;
    float s[NT], q[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) s[t] = q[t] = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int mm = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (mm < M) {
            int64_t orow = mm;
            if (DECONV) {
                const int ob = mm / (RH * RW), op = mm - ob * (RH * RW), oh = op / RW, ow = op - oh * RW;
                orow = ((int64_t)ob * g.Ho + g.s * oh + zi) * g.Wo + g.s * ow + zj;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float v = acc[t][i];
                y[orow * ldy + coff + n0 + 32 * t + r] = v;
                s[t] += v;
                q[t] = fmaf(v, v, q[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
        c2d_block_sums(s[t], q[t], part + ((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * 2 * g.Cout, g.Cout, n0 + 32 * t);
}

// ---- backward: dX -------------------------------------------------------------------------------------------------------------------------
template <bool DECONV, int NT>
__global__ __launch_bounds__(C2_T) void c2d_dx_kernel(const float *__restrict__ dz, const float *__restrict__ y, int ld, int coff, C2Norm nm,
                                                     const float *__restrict__ wt, C2Geo g, const float *__restrict__ addend, C2Prev pv,
                                                     float *__restrict__ out, float *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int M = g.B * g.H * g.W;
    const int m0 = (blockIdx.x * 4 + wv) * 32, m = m0 + r, n0 = blockIdx.y * (32 * NT);
    const bool live = m < M;
    const int mc = live ? m : 0;
    const int b = mc / (g.H * g.W), p = mc - b * (g.H * g.W), ph = p / g.W, pw = p - ph * g.W;
    const int taps = DECONV ? g.s * g.s : 9;
    const float *wr = wt + ((int64_t)(n0 + r) * taps) * g.Cout + 8 * h;
    const int64_t wstep = (int64_t)32 * taps * g.Cout;                                     // to the next column block
    floatx16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    // (the channel block is the outer loop: the layer's five constants are loaded once for all taps)
    for (int c = 0; c < g.Cout; c += 16) {
        float mu[8], is[8], sc[8], k1[8], k2[8];
        c2d_ld8(nm.mean + c + 8 * h, mu);
        c2d_ld8(nm.invstd + c + 8 * h, is);
        c2d_ld8(nm.scale + c + 8 * h, sc);
        c2d_ld8(nm.c1 + c + 8 * h, k1);
        c2d_ld8(nm.c2 + c + 8 * h, k2);
        for (int tap = 0; tap < taps; ++tap) {
            bool valid;
            int src;
            if (DECONV) {
                const int ti = tap / g.s, tj = tap - ti * g.s;
                valid = live;
                src = (b * g.Ho + g.s * ph + ti) * g.Wo + g.s * pw + tj;
            } else {
                const int ty = tap / 3, tx = tap - 3 * ty;
                const int nh = ph + 1 - ty, nw = pw + 1 - tx;                              // s x the output position this tap came from
                const int qh = (nh > 0 ? nh : 0) / g.s, qw = (nw > 0 ? nw : 0) / g.s;
                valid = live && nh >= 0 && nw >= 0 && qh * g.s == nh && qw * g.s == nw && qh < g.Ho && qw < g.Wo;    // parity and halo: selected
                src = (b * g.Ho + qh) * g.Wo + qw;
            }
            src = valid ? src : 0;                                                         // (reads pixel 0 and selects nothing)
            const int64_t at = (int64_t)src * ld + coff + 8 * h + c;
            float av[8], yv[8];
            c2d_ld8(dz + at, av);
            c2d_ld8(y + at, yv);
#pragma unroll
            for (int j = 0; j < 8; ++j) av[j] = valid ? sc[j] * ((av[j] - k1[j]) - ((yv[j] - mu[j]) * is[j]) * k2[j]) : 0.f;
            bf16x8 ap[3];
            split8(av, ap);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float bv[8];
                bf16x8 bp[3];
                c2d_ld8(wr + t * wstep + tap * g.Cout + c, bv);
                split8(bv, bp);
                acc[t] = mfma_bf16x3(ap, bp, acc[t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) c2d_mfma_drain(acc[t]);
    const bool prev = pv.y != nullptr;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int cc = n0 + 32 * t + r;
        const float psc = prev ? pv.scale[cc] : 0.f, psh = prev ? pv.shift[cc] : 0.f, pmu = prev ? pv.mean[cc] : 0.f, pis = prev ? pv.invstd[cc] : 0.f;
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int mm = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (mm < M) {
                const int64_t o = (int64_t)mm * g.Cin + cc;
                float v = acc[t][i];
                if (addend) v += addend[o];
                if (prev) {
                    const float yp = pv.y[o];
                    v = fmaf(psc, yp, psh) > 0.f ? v : 0.f;
                    s += v;
                    q = fmaf(v, (yp - pmu) * pis, q);
                }
                out[o] = v;
            }
        }
        if (prev) c2d_block_sums(s, q, part + (int64_t)blockIdx.x * 2 * g.Cin, g.Cin, n0 + 32 * t);      // (kernel-uniform)
    }
}

// ---- backward: dW -------------------------------------------------------------------------------------------------------------------------
// wave = tap (4 blockIdx.z + wave), blockIdx.x = rows rpc t .. of the OUTPUT pixels (deconv: of the input pixels), blockIdx.y = (co block, ci block).
// A[row r = co][k = row] = dY, B[k = row][col r = ci] = the activated input under the tap.
template <bool NORM, bool DECONV>
__global__ __launch_bounds__(C2_T) void c2d_dw_kernel(const float *__restrict__ dz, const float *__restrict__ y, int ld, int coff, C2Norm nm,
                                                     const float *__restrict__ x, const float *__restrict__ sc_in, const float *__restrict__ sh_in,
                                                     C2Geo g, int rpc, float *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int taps = DECONV ? g.s * g.s : 9;
    const int tap = blockIdx.z * 4 + wv;
    if (tap >= taps) return;                                        // (wave-uniform; no barrier below)
    const int ncb = g.Cin / 32, co0 = (blockIdx.y / ncb) * 32, ci0 = (blockIdx.y % ncb) * 32;
    const int RH = DECONV ? g.H : g.Ho, RW = DECONV ? g.W : g.Wo, M = g.B * RH * RW;
    const int r0 = blockIdx.x * rpc, r1 = min(r0 + rpc, M);
    const int t1 = DECONV ? tap / g.s : tap / 3, t2 = DECONV ? tap - t1 * g.s : tap - 3 * t1;
    const int co = co0 + r, ci = ci0 + r;
    const float mu = nm.mean[co], is = nm.invstd[co], sc = nm.scale[co], k1 = nm.c1[co], k2 = nm.c2[co];
    const float sci = NORM ? sc_in[ci] : 1.f, shi = NORM ? sh_in[ci] : 0.f;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int ks = r0; ks < r1; ks += 16) {
        const int mb = ks + 8 * h, mbc = mb < r1 ? mb : r0;
        int b = mbc / (RH * RW);
        const int p = mbc - b * (RH * RW);
        int ph = p / RW, pw = p - ph * RW;
        float av[8], bv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = mb + j < r1;
            const int bb = in ? b : 0, hh = in ? ph : 0, ww = in ? pw : 0;                 // (a padding row reads pixel 0 and selects nothing)
            int64_t dyrow, arow;
            bool valid;
            if (DECONV) {
                dyrow = ((int64_t)bb * g.Ho + g.s * hh + t1) * g.Wo + g.s * ww + t2;
                arow = ((int64_t)bb * g.H + hh) * g.W + ww;
                valid = true;
            } else {
                const int hi = hh * g.s + t1 - 1, wi = ww * g.s + t2 - 1;
                valid = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
                dyrow = ((int64_t)bb * g.Ho + hh) * g.Wo + ww;
                arow = valid ? ((int64_t)bb * g.H + hi) * g.W + wi : 0;
            }
            const float d = dz[dyrow * ld + coff + co], yv = y[dyrow * ld + coff + co];
            const float xv = x[arow * g.Cin + ci];
            const float a = NORM ? relu_np(fmaf(sci, xv, shi)) : xv;
            av[j] = in ? sc * ((d - k1) - ((yv - mu) * is) * k2) : 0.f;
            bv[j] = (in && valid) ? a : 0.f;
            // the next row of the row-major (b, h, w) order
            const bool wrapw = pw + 1 == RW, wraph = wrapw && ph + 1 == RH;
            pw = wrapw ? 0 : pw + 1;
            ph = wraph ? 0 : (wrapw ? ph + 1 : ph);
            b = wraph ? b + 1 : b;
        }
        acc = c2d_step(av, bv, acc);
    }
    c2d_mfma_drain(acc);
    float *pt = part + (int64_t)blockIdx.x * g.Cout * g.Cin * taps;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int rr = co0 + (i & 3) + 8 * (i >> 2) + 4 * h;       // the accumulator row: co
        if (DECONV) pt[((int64_t)ci * g.Cout + rr) * taps + tap] = acc[i];
        else pt[((int64_t)rr * g.Cin + ci) * taps + tap] = acc[i];
    }
}

// ---- the concat buffer's backward entry -----------------------------------------------------------------------------------------------------
// workgroup = C2_RB_ROWS rows; thread = channels t, t + 256, ..., each summed over the rows in row order
__global__ __launch_bounds__(C2_T) void c2d_relu_bwd_kernel(const float *__restrict__ gout, const float *__restrict__ y, const float *__restrict__ mean,
                                                           const float *__restrict__ invstd, const float *__restrict__ scale,
                                                           const float *__restrict__ shift, int64_t M, int C, int64_t ld, int coff,
                                                           float *__restrict__ dz, float *__restrict__ part)
{
    const int64_t r0 = (int64_t)blockIdx.x * C2_RB_ROWS, r1 = r0 + C2_RB_ROWS < M ? r0 + C2_RB_ROWS : M;
    for (int c = threadIdx.x; c < C; c += C2_T) {
        const float mu = mean[c], is = invstd[c], sc = scale[c], sh = shift[c];
        float s = 0.f, q = 0.f;
        for (int64_t m = r0; m < r1; ++m) {
            const int64_t o = m * ld + coff + c;
            const float yv = y[o];
            const float d = fmaf(sc, yv, sh) > 0.f ? gout[o] : 0.f;
            dz[o] = d;
            s += d;
            q = fmaf(d, (yv - mu) * is, q);
        }
        part[(int64_t)blockIdx.x * 2 * C + c] = s;
        part[(int64_t)blockIdx.x * 2 * C + C + c] = q;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
static bool c2d_width_ok(int C) { return C >= 32 && C <= C2_CMAX && C % 32 == 0; }

static int c2d_geo(const char *who, bool deconv, int B, int H, int W, int Cin, int Cout, int s, C2Geo &g)
{
    PAPC_REQUIRE(c2d_width_ok(Cin) && c2d_width_ok(Cout), PAPC_E_UNSUPPORTED, "%s: Cin=%d Cout=%d (multiples of 32 up to %d)", who, Cin, Cout, C2_CMAX);
    if (deconv) PAPC_REQUIRE(s == 1 || s == 2 || s == 4, PAPC_E_UNSUPPORTED, "%s: stride %d (the deconvolution's kernel = stride is 1, 2 or 4)", who, s);
    else PAPC_REQUIRE(s == 1 || s == 2, PAPC_E_UNSUPPORTED, "%s: stride %d (1 or 2)", who, s);
    PAPC_REQUIRE(B >= 1 && H >= 1 && W >= 1, PAPC_E_INVALID, "%s: B=%d H=%d W=%d", who, B, H, W);
    g.B = B; g.H = H; g.W = W; g.s = s; g.Cin = Cin; g.Cout = Cout;
    g.Ho = deconv ? s * H : (H - 1) / s + 1;
    g.Wo = deconv ? s * W : (W - 1) / s + 1;
    const int64_t big = std::max((int64_t)B * H * W, (int64_t)B * g.Ho * g.Wo);
    PAPC_REQUIRE(big < ((int64_t)1 << 31) / 4, PAPC_E_INVALID, "%s: B=%d H=%d W=%d (at most 2^29 pixels)", who, B, H, W);
    return PAPC_OK;
}

static int c2d_dw_rpc(int64_t M)
{
    const int64_t rpc = cdiv(cdiv(M, C2_DW_CHUNKS), 16) * 16;
    return (int)std::max<int64_t>(256, rpc);
}

static size_t c2d_dw_ws(const C2Geo &g, bool deconv)
{
    const int64_t M = deconv ? (int64_t)g.B * g.H * g.W : (int64_t)g.B * g.Ho * g.Wo;
    const int taps = deconv ? g.s * g.s : 9;
    return (size_t)cdiv(M, c2d_dw_rpc(M)) * g.Cout * g.Cin * taps * sizeof(float);
}

static bool c2d_aligned(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr, const void *e = nullptr,
                        const void *f = nullptr, const void *g = nullptr, const void *h = nullptr)
{
    return aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d) && aligned16(e) && aligned16(f) && aligned16(g) && aligned16(h);
}

static int c2d_fwd(const char *who, bool deconv, const float *x, const float *sc_in, const float *sh_in, const float *wk, int B, int H, int W, int Cin,
                   int Cout, int s, float *y, int64_t ldy, int coff, float *part, papc_stream_t stream)
{
    C2Geo g;
    const int err = c2d_geo(who, deconv, B, H, W, Cin, Cout, s, g);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(x && wk && y && part && (sc_in == nullptr) == (sh_in == nullptr), PAPC_E_INVALID, "%s: null pointer (scale and shift go together)", who);
    PAPC_REQUIRE(c2d_aligned(x, sc_in, sh_in, wk), PAPC_E_INVALID, "%s: x, scale, shift and wk must be 16-byte aligned", who);
    PAPC_REQUIRE(ldy >= coff + Cout && coff >= 0 && ldy < ((int64_t)1 << 20), PAPC_E_INVALID, "%s: ldy=%lld coff=%d Cout=%d", who, (long long)ldy, coff, Cout);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MLP_GEMM, st);
    const int64_t M = deconv ? (int64_t)B * H * W : (int64_t)B * g.Ho * g.Wo;
    const int nt = Cout % 64 == 0 ? 2 : 1;                                                 // column blocks per wave
    const dim3 grid((unsigned)cdiv(M, 128), (unsigned)(Cout / (32 * nt)), deconv ? (unsigned)(s * s) : 1u);
#define C2D_FWD(NORM, DEC, NT_) hipLaunchKernelGGL((c2d_fwd_kernel<NORM, DEC, NT_>), grid, dim3(C2_T), 0, st, x, sc_in, sh_in, wk, g, y, (int)ldy, coff, part)
#define C2D_FWD_NT(NORM, DEC) do { if (nt == 2) C2D_FWD(NORM, DEC, 2); else C2D_FWD(NORM, DEC, 1); } while (0)
    if (deconv) {
        if (sc_in) C2D_FWD_NT(true, true);
        else C2D_FWD_NT(false, true);
    } else {
        if (sc_in) C2D_FWD_NT(true, false);
        else C2D_FWD_NT(false, false);
    }
#undef C2D_FWD_NT
#undef C2D_FWD
    return check_launch(who);
}

static int c2d_dx(const char *who, bool deconv, const float *dz, const float *y, int64_t ld, int coff, const C2Norm &nm, const float *wt, int B, int H,
                  int W, int Cin, int Cout, int s, const float *addend, const C2Prev &pv, float *out, float *part, papc_stream_t stream)
{
    C2Geo g;
    const int err = c2d_geo(who, deconv, B, H, W, Cin, Cout, s, g);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(dz && y && nm.mean && nm.invstd && nm.scale && nm.c1 && nm.c2 && wt && out, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(!pv.y || (pv.mean && pv.invstd && pv.scale && pv.shift && part), PAPC_E_INVALID,
                 "%s: y_prev needs its mean, invstd, scale, shift and red_partial", who);
    PAPC_REQUIRE(c2d_aligned(dz, y, wt, nm.mean, nm.invstd, nm.scale, nm.c1, nm.c2), PAPC_E_INVALID, "%s: dz, y, wt and the constants must be 16-byte aligned", who);
    PAPC_REQUIRE(ld >= coff + Cout && coff >= 0 && coff % 4 == 0 && ld % 4 == 0 && ld < ((int64_t)1 << 20), PAPC_E_INVALID,
                 "%s: ld=%lld coff=%d Cout=%d (multiples of 4)", who, (long long)ld, coff, Cout);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_BWD_DX, st);
    const int nt = Cin % 64 == 0 ? 2 : 1;                                                  // column blocks per wave
    const dim3 grid((unsigned)cdiv((int64_t)B * H * W, 128), (unsigned)(Cin / (32 * nt)));
#define C2D_DX(DEC, NT_) hipLaunchKernelGGL((c2d_dx_kernel<DEC, NT_>), grid, dim3(C2_T), 0, st, dz, y, (int)ld, coff, nm, wt, g, addend, pv, out, part)
    if (deconv) {
        if (nt == 2) C2D_DX(true, 2);
        else C2D_DX(true, 1);
    } else {
        if (nt == 2) C2D_DX(false, 2);
        else C2D_DX(false, 1);
    }
#undef C2D_DX
    return check_launch(who);
}

static int c2d_dw(const char *who, bool deconv, const float *dz, const float *y, int64_t ld, int coff, const C2Norm &nm, const float *x,
                  const float *sc_in, const float *sh_in, int B, int H, int W, int Cin, int Cout, int s, float *dw, int accumulate, void *workspace,
                  size_t workspace_bytes, papc_stream_t stream)
{
    C2Geo g;
    const int err = c2d_geo(who, deconv, B, H, W, Cin, Cout, s, g);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(dz && y && nm.mean && nm.invstd && nm.scale && nm.c1 && nm.c2 && x && dw && workspace && (sc_in == nullptr) == (sh_in == nullptr),
                 PAPC_E_INVALID, "%s: null pointer (scale and shift go together)", who);
    PAPC_REQUIRE(ld >= coff + Cout && coff >= 0 && ld < ((int64_t)1 << 20), PAPC_E_INVALID, "%s: ld=%lld coff=%d Cout=%d", who, (long long)ld, coff, Cout);
    const size_t need = c2d_dw_ws(g, deconv);
    PAPC_REQUIRE(workspace_bytes >= need && aligned16(workspace), PAPC_E_INVALID, "%s: workspace %zu bytes < %zu (or not 16-byte aligned)", who, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const int64_t M = deconv ? (int64_t)B * H * W : (int64_t)B * g.Ho * g.Wo;
    const int rpc = c2d_dw_rpc(M), T = (int)cdiv(M, rpc), taps = deconv ? s * s : 9;
    float *part = static_cast<float *>(workspace);
    {
        ProfScope prof(PAPC_K_BWD_DW, st);
        const dim3 grid((unsigned)T, (unsigned)((Cout / 32) * (Cin / 32)), (unsigned)cdiv(taps, 4));
        if (deconv) {
            if (sc_in) hipLaunchKernelGGL((c2d_dw_kernel<true, true>), grid, dim3(C2_T), 0, st, dz, y, (int)ld, coff, nm, x, sc_in, sh_in, g, rpc, part);
            else hipLaunchKernelGGL((c2d_dw_kernel<false, true>), grid, dim3(C2_T), 0, st, dz, y, (int)ld, coff, nm, x, sc_in, sh_in, g, rpc, part);
        } else {
            if (sc_in) hipLaunchKernelGGL((c2d_dw_kernel<true, false>), grid, dim3(C2_T), 0, st, dz, y, (int)ld, coff, nm, x, sc_in, sh_in, g, rpc, part);
            else hipLaunchKernelGGL((c2d_dw_kernel<false, false>), grid, dim3(C2_T), 0, st, dz, y, (int)ld, coff, nm, x, sc_in, sh_in, g, rpc, part);
        }
        const int e = check_launch(who);
        if (e != PAPC_OK) return e;
    }
    return papc_reduce_partials_f32(part, T, (int64_t)Cout * Cin * taps, dw, accumulate, stream);      // the chunks in chunk order (fold.h)
}

}  // namespace papc

using namespace papc;

extern "C" {

int papc_conv2d_ok(int Cin, int Cout, int stride, int H, int W)
{
    C2Geo g;
    return c2d_geo("papc_conv2d_ok", false, 1, H, W, Cin, Cout, stride, g) == PAPC_OK ? 1 : 0;
}

int papc_deconv2d_ok(int Cin, int Cout, int stride)
{
    C2Geo g;
    return c2d_geo("papc_deconv2d_ok", true, 1, 1, 1, Cin, Cout, stride, g) == PAPC_OK ? 1 : 0;
}

int papc_conv2d_parts(int64_t M) { return M >= 1 && M < ((int64_t)1 << 31) ? (int)cdiv(M, 128) : 0; }

int papc_conv2d_prep_f32(const float *const *w, float *const *wk, float *const *wt, const int *cin, const int *cout, const int *stride, const int *deconv,
                         int count, papc_stream_t stream)
{
    const char *who = "papc_conv2d_prep_f32";
    PAPC_REQUIRE(w && wk && wt && cin && cout && stride && deconv, PAPC_E_INVALID, "%s: null array", who);
    PAPC_REQUIRE(count >= 1 && count <= C2_PREP_MAX, PAPC_E_INVALID, "%s: count=%d not in [1, %d]", who, count, C2_PREP_MAX);
    C2PrepJobs jb;
    memset(&jb, 0, sizeof(jb));
    int nmax = 0;
    for (int i = 0; i < count; ++i) {
        C2Geo g;
        const int err = c2d_geo(who, deconv[i] != 0, 1, 1, 1, cin[i], cout[i], stride[i], g);
        if (err != PAPC_OK) return err;
        PAPC_REQUIRE(w[i] && wk[i] && wt[i] && aligned16(wk[i]) && aligned16(wt[i]), PAPC_E_INVALID, "%s: null or misaligned pointer in job %d", who, i);
        jb.w[i] = w[i]; jb.wk[i] = wk[i]; jb.wt[i] = wt[i]; jb.cin[i] = cin[i]; jb.cout[i] = cout[i];
        jb.taps[i] = deconv[i] ? stride[i] * stride[i] : 9;
        jb.deconv[i] = deconv[i] ? 1 : 0;
        nmax = std::max(nmax, cin[i] * cout[i] * jb.taps[i]);
    }
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(c2d_prep_kernel, dim3((unsigned)cdiv(nmax, C2_T), (unsigned)count), dim3(C2_T), 0, st, jb);
    return check_launch(who);
}

int papc_conv2d_fwd_f32(const float *x, const float *scale_in, const float *shift_in, const float *wk, int B, int H, int W, int Cin, int Cout, int stride,
                        float *y, float *stats_partial, papc_stream_t stream)
{
    return c2d_fwd("papc_conv2d_fwd_f32", false, x, scale_in, shift_in, wk, B, H, W, Cin, Cout, stride, y, Cout, 0, stats_partial, stream);
}

int papc_conv2d_bwd_dx_f32(const float *dz, const float *y, const float *mean, const float *invstd, const float *scale, const float *c1, const float *c2,
                           const float *wt, int B, int H, int W, int Cin, int Cout, int stride, const float *addend, const float *y_prev,
                           const float *mean_prev, const float *invstd_prev, const float *scale_prev, const float *shift_prev, float *dx,
                           float *red_partial, papc_stream_t stream)
{
    const C2Norm nm = {mean, invstd, scale, c1, c2};
    const C2Prev pv = {y_prev, mean_prev, invstd_prev, scale_prev, shift_prev};
    return c2d_dx("papc_conv2d_bwd_dx_f32", false, dz, y, Cout, 0, nm, wt, B, H, W, Cin, Cout, stride, addend, pv, dx, red_partial, stream);
}

size_t papc_conv2d_bwd_dw_workspace(int B, int H, int W, int Cin, int Cout, int stride)
{
    C2Geo g;
    if (c2d_geo("papc_conv2d_bwd_dw_workspace", false, B, H, W, Cin, Cout, stride, g) != PAPC_OK) return 0;
    return c2d_dw_ws(g, false);
}

int papc_conv2d_bwd_dw_f32(const float *dz, const float *y, const float *mean, const float *invstd, const float *scale, const float *c1, const float *c2,
                           const float *x, const float *scale_in, const float *shift_in, int B, int H, int W, int Cin, int Cout, int stride, float *dw,
                           int accumulate, void *workspace, size_t workspace_bytes, papc_stream_t stream)
{
    const C2Norm nm = {mean, invstd, scale, c1, c2};
    return c2d_dw("papc_conv2d_bwd_dw_f32", false, dz, y, Cout, 0, nm, x, scale_in, shift_in, B, H, W, Cin, Cout, stride, dw, accumulate, workspace,
                  workspace_bytes, stream);
}

int papc_deconv2d_fwd_f32(const float *x, const float *scale_in, const float *shift_in, const float *wk, int B, int H, int W, int Cin, int Cout, int stride,
                          float *y, int64_t ldy, int coff, float *stats_partial, papc_stream_t stream)
{
    return c2d_fwd("papc_deconv2d_fwd_f32", true, x, scale_in, shift_in, wk, B, H, W, Cin, Cout, stride, y, ldy, coff, stats_partial, stream);
}

int papc_deconv2d_bwd_dx_f32(const float *dz, const float *y, int64_t ld, int coff, const float *mean, const float *invstd, const float *scale,
                             const float *c1, const float *c2, const float *wt, int B, int H, int W, int Cin, int Cout, int stride, const float *addend,
                             const float *y_prev, const float *mean_prev, const float *invstd_prev, const float *scale_prev, const float *shift_prev,
                             float *dx, float *red_partial, papc_stream_t stream)
{
    const C2Norm nm = {mean, invstd, scale, c1, c2};
    const C2Prev pv = {y_prev, mean_prev, invstd_prev, scale_prev, shift_prev};
    return c2d_dx("papc_deconv2d_bwd_dx_f32", true, dz, y, ld, coff, nm, wt, B, H, W, Cin, Cout, stride, addend, pv, dx, red_partial, stream);
}

size_t papc_deconv2d_bwd_dw_workspace(int B, int H, int W, int Cin, int Cout, int stride)
{
    C2Geo g;
    if (c2d_geo("papc_deconv2d_bwd_dw_workspace", true, B, H, W, Cin, Cout, stride, g) != PAPC_OK) return 0;
    return c2d_dw_ws(g, true);
}

int papc_deconv2d_bwd_dw_f32(const float *dz, const float *y, int64_t ld, int coff, const float *mean, const float *invstd, const float *scale,
                             const float *c1, const float *c2, const float *x, const float *scale_in, const float *shift_in, int B, int H, int W, int Cin,
                             int Cout, int stride, float *dw, int accumulate, void *workspace, size_t workspace_bytes, papc_stream_t stream)
{
    const C2Norm nm = {mean, invstd, scale, c1, c2};
    return c2d_dw("papc_deconv2d_bwd_dw_f32", true, dz, y, ld, coff, nm, x, scale_in, shift_in, B, H, W, Cin, Cout, stride, dw, accumulate, workspace,
                  workspace_bytes, stream);
}

int papc_conv2d_relu_bwd_parts(int64_t M) { return M >= 1 && M < ((int64_t)1 << 31) ? (int)cdiv(M, C2_RB_ROWS) : 0; }

int papc_conv2d_relu_bwd_f32(const float *gout, const float *y, int64_t ld, int coff, const float *mean, const float *invstd, const float *scale,
                             const float *shift, int64_t M, int C, float *dz, float *red_partial, papc_stream_t stream)
{
    const char *who = "papc_conv2d_relu_bwd_f32";
    PAPC_REQUIRE(gout && y && mean && invstd && scale && shift && dz && red_partial, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(M >= 1 && M < ((int64_t)1 << 31) && C >= 1 && C <= 4096 && coff >= 0 && ld >= coff + C, PAPC_E_INVALID, "%s: M=%lld C=%d ld=%lld coff=%d", who,
                 (long long)M, C, (long long)ld, coff);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_BWD_REDUCE, st);
    hipLaunchKernelGGL(c2d_relu_bwd_kernel, dim3((unsigned)cdiv(M, C2_RB_ROWS)), dim3(C2_T), 0, st, gout, y, mean, invstd, scale, shift, M, C, ld, coff, dz, red_partial);
    return check_launch(who);
}

}  // extern "C"
