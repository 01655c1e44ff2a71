// voxconv.hip -- the VoxNet backbone as implicit-GEMM 3-D convolutions, for gfx950, with the head's LeakyReLU + dropout and the occupancy grid.
//
// Reference: PAPC/models/classify/voxnet/voxnet.py:7-25
//     Conv3D(1, 32, 5, stride 2) -> BatchNorm(32) -> LeakyReLU -> Conv3D(32, 32, 3) -> MaxPool3D(2, 2) -> reshape(-1, 32 * 6^3) -> head
// For an input edge E: E1 = (E - 5) / 2 + 1 (conv1), E2 = E1 - 2 (conv2), Ep = E2 / 2 (pool); the model has E = 32 -> 14, 12, 6.
//
// Layout: activations are channel-last rows, y1 [B E1^3, 32] (the PRE-norm conv1 output, row = ((b E1 + z) E1 + y) E1 + x).  The weights keep
// the source's shapes ([32,1,5,5,5], [32,32,3,3,3]); the K order of every product is tap-major, k = tap * Cin + ci, tap = (tz K + ty) K + tx.
// vox_w2_prep_kernel writes W2 once per step in the two K-major orders the conv2 kernels read ([co][tap][ci] and [ci][tap][co], 2 x 110 KB).
//
// Every kernel below is a wave per 32 x 32 output block of v_mfma_f32_32x32x16_bf16 through bf16x3.h (fp32 accuracy, fp32 accumulation): lane
// (r = lane & 31, h = lane >> 5) holds A[row r][k = 8h + j] and B[k = 8h + j][col r], the accumulator register i is row (i & 3) + 8 (i >> 2) + 4h
// of column r.  The operands are gathered from global memory (L2-resident: the whole y1 of a cloud is 351 KB) by the im2col addressing; the
// [B E2^3, 32] pre-pool tensor, the dense pool gradient and the LeakyReLU mask are never stored.
//
//   vox_conv1_fwd_kernel   M = B E1^3 rows, K = 125 taps padded to 128 with exact zeros, N = 32.  A = the input patch through a tap -> offset table
//                         in LDS.  Epilogue: + bias, y1, and sum y / sum y^2 per channel, one partial row [2][32] per workgroup (128 rows) -- the
//                         layout papc_bn_finalize_f32 folds in tile order.
//   vox_conv2_pool_kernel  K = 27 x 32, N = 32, A = leaky(scale y1 + shift) on load.  A tile's 32 rows are FOUR 2x2x2 pool groups ordered so that
//                         a group's eight members are registers of one lane: row rho is member (rho & 3) + 4 ((rho >> 3) & 1) of group
//                         2 ((rho >> 2) & 1) + (rho >> 4), i.e. lane half h holds groups 2h (registers 0..7) and 2h + 1 (registers 8..15), member
//                         e = dz 4 + dy 2 + dx in register (e & 3) + 4 (e >> 2).  Epilogue: + bias, max in member order (first on an exact tie, a
//                         NaN goes through), winner byte [group][32], value into the source's flatten order out[b][c Ep^3 + p].
//   vox_conv2_dx_kernel    dA1[b, p, ci] = sum_tap sum_co dY[b, p - tap, co] W2[co, ci, tap] over the rows of y1; dY formed on load from the pooled
//                         gradient (channel-last copy gp [B Ep^3, 32]) and the winner bytes; positions outside the E2 grid are the zero halo.
//                         Epilogue: x LeakyReLU' (sign of scale y1 + shift, recomputed) -> dz, and sum dz / sum dz xhat per workgroup -- the layout
//                         papc_bn_bwd_finalize_f32 folds.
//   vox_conv2_dw_kernel    dW2[co, ci, tap] = sum_rows dY[row, co] a1[row + tap, ci]: wave = tap, workgroup column = chunk of VX_DWG pool groups;
//                         a k step is two groups' eight members.  Partials in the source's [co][ci][tap] order, folded in chunk order.
//   vox_conv1_dw_kernel    dW1[co, tap] = sum_rows dy1[row, co] x[patch(row), tap], dy1 = scale (dz - c1 - xhat c2) on load; wave = 32 taps, chunk =
//                         VX_W1CH rows.  Folded in chunk order.  conv1.bias feeds a train-mode norm: its gradient is the exact 0.
// No float atomics, every cross-workgroup sum a fixed-order fold (fold.h): two runs are bit-identical.  Plain C++ loads and stores only.
// Every k loop is straight-line -- an operand is always loaded, from an address that exists, and then selected; no branch, per lane or per wave,
// stands around an MFMA -- so the accumulator stays in its AGPRs from the first product to vox_mfma_drain (a tap skipped with
// __ballot + continue made hipcc copy the accumulator out across the loop's back edge too soon after the last MFMA).
#include "bf16x3.h"
#include "fold.h"
#include "hashrng.h"

namespace papc {

constexpr int VX_T = 256;        // threads of every MFMA kernel here (4 waves)
constexpr int VX_C = 32;         // channels of both convs
constexpr int VX_K1 = 125;       // conv1 taps
constexpr int VX_K2 = 27;        // conv2 taps
constexpr int VX_W2N = VX_C * VX_C * VX_K2;   // 27648
constexpr int VX_DWG = 64;       // pool groups per dW2 chunk (32 k steps)
constexpr int VX_W1CH = 256;     // rows per dW1 chunk (16 k steps)
constexpr float VX_SLOPE = 0.01f;   // nn.LeakyReLU's default

struct VxGeo { int B, E, E1, E2, Ep, M1, NG; };     // M1 = B E1^3 rows of y1, NG = B Ep^3 pool groups

__device__ __forceinline__ floatx16 vox_step(const float (&av)[8], const float (&bv)[8], floatx16 acc)
{
    bf16x8 ap[3], bp[3];
    split8(av, ap);
    split8(bv, bp);
    return mfma_bf16x3(ap, bp, acc);
}

__device__ __forceinline__ void vox_ld8(const float *p, float (&v)[8])
{
    const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// Behind a k loop, in front of the epilogue's first read of the accumulator: the last MFMA's passes are over whatever block layout the compiler
// chose (an epilogue must not lean on wait states counted across a loop's back edge).
__device__ __forceinline__ void vox_mfma_drain(floatx16 &acc)
{
    asm volatile("s_nop 15" : "+a"(acc));                // (the accumulator stays in its AGPRs up to here: every copy out of them comes after)
}

__device__ __forceinline__ float vox_leaky(float t) { return t > 0.f ? t : VX_SLOPE * t; }

// the per-channel sums (s, q) of a workgroup's four waves -> part[blockIdx.x][2][32]; s, q: the lane's sums over its 16 registers
__device__ __forceinline__ void vox_block_sums(float s, float q, float *__restrict__ part)
{
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    s += __shfl_xor(s, 32);                              // the two row halves of the lane pair
    q += __shfl_xor(q, 32);
    if (lane < 32) { red[wv][lane] = s; red[wv][32 + lane] = q; }
    __syncthreads();
    if (threadIdx.x < 64) part[(int64_t)blockIdx.x * 64 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// ---- conv1 forward ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_T) void vox_conv1_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w1, const float *__restrict__ bias,
                                                            VxGeo g, float *__restrict__ y1, float *__restrict__ part)
{
    __shared__ int toff[128];
    if (threadIdx.x < 128) {
        const int k = threadIdx.x < VX_K1 ? threadIdx.x : 0;
        toff[threadIdx.x] = ((k / 25) * g.E + (k / 5) % 5) * g.E + k % 5;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int m0 = (blockIdx.x * 4 + wv) * 32, m = m0 + r;
    const bool live = m < g.M1;
    const int e13 = g.E1 * g.E1 * g.E1, mc = live ? m : 0;
    const int b = mc / e13, p = mc - b * e13, z = p / (g.E1 * g.E1), yy = (p / g.E1) % g.E1, xx = p % g.E1;
    const float *xb = x + (int64_t)b * g.E * g.E * g.E + ((2 * z) * g.E + 2 * yy) * g.E + 2 * xx;
    const float *wr = w1 + r * VX_K1;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 2
    for (int ks = 0; ks < 8; ++ks) {
        float av[8], bv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 16 * ks + 8 * h + j;
            const bool in = k < VX_K1;
            const float xv = xb[toff[k]], wv = wr[in ? k : 0];     // (always loaded, from addresses that exist: no branch around the MFMAs)
            av[j] = (live && in) ? xv : 0.f;
            bv[j] = in ? wv : 0.f;
        }
        acc = vox_step(av, bv, acc);
    }
    vox_mfma_drain(acc);
    const float bc = bias ? bias[r] : 0.f;
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int mm = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (mm < g.M1) {
            const float v = acc[i] + bc;
            y1[(int64_t)mm * VX_C + r] = v;
            s += v;
            q = fmaf(v, v, q);
        }
    }
    vox_block_sums(s, q, part);
}

// ---- W2 in the two K-major orders ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_T) void vox_w2_prep_kernel(const float *__restrict__ w2, float *__restrict__ wk, float *__restrict__ wt)
{
    const int i = blockIdx.x * VX_T + threadIdx.x;
    if (i >= VX_W2N) return;
    const int co = i / (VX_C * VX_K2), rem = i - co * (VX_C * VX_K2), ci = rem / VX_K2, tap = rem - ci * VX_K2;
    const float v = w2[i];
    wk[co * (VX_C * VX_K2) + tap * VX_C + ci] = v;
    wt[ci * (VX_C * VX_K2) + tap * VX_C + co] = v;
}

// ---- conv2 + pool forward -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_T) void vox_conv2_pool_kernel(const float *__restrict__ y1, const float *__restrict__ scale, const float *__restrict__ shift,
                                                             const float *__restrict__ wk, const float *__restrict__ bias, VxGeo g,
                                                             float *__restrict__ out, unsigned char *__restrict__ win)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int G0 = (blockIdx.x * 4 + wv) * 4;
    if (G0 >= g.NG) return;                                         // (wave-uniform; no barrier below)
    const int ep3 = g.Ep * g.Ep * g.Ep, e1 = g.E1;
    // this lane's A row: member e of group G0 + gi
    const int gi = 2 * ((r >> 2) & 1) + (r >> 4), e = (r & 3) + 4 * ((r >> 3) & 1);
    const int Gc = G0 + gi < g.NG ? G0 + gi : 0;                    // (a padding group reads group 0 and stores nothing)
    const int b = Gc / ep3, p = Gc - b * ep3, pz = p / (g.Ep * g.Ep), py = (p / g.Ep) % g.Ep, px = p % g.Ep;
    const int row0 = ((b * e1 + 2 * pz + (e >> 2)) * e1 + 2 * py + ((e >> 1) & 1)) * e1 + 2 * px + (e & 1);
    const float *ar = y1 + (int64_t)row0 * VX_C + 8 * h;
    const float *wr = wk + r * (VX_C * VX_K2) + 8 * h;
    float sc[2][8], sh[2][8];
#pragma unroll
    for (int q = 0; q < 2; ++q) { vox_ld8(scale + 16 * q + 8 * h, sc[q]); vox_ld8(shift + 16 * q + 8 * h, sh[q]); }
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int tz = 0; tz < 3; ++tz)
        for (int ty = 0; ty < 3; ++ty)
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) {
                const int tap = (tz * 3 + ty) * 3 + tx, to = (tz * e1 + ty) * e1 + tx;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    float av[8], bv[8];
                    vox_ld8(ar + (int64_t)to * VX_C + 16 * q, av);
                    vox_ld8(wr + tap * VX_C + 16 * q, bv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) av[j] = vox_leaky(fmaf(sc[q][j], av[j], sh[q][j]));
                    acc = vox_step(av, bv, acc);
                }
            }
    vox_mfma_drain(acc);
    const float bc = bias ? bias[r] : 0.f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int G = G0 + 2 * h + half;
        if (G >= g.NG) continue;
        float best = acc[8 * half] + bc;
        unsigned wb = 0;
#pragma unroll
        for (int m = 1; m < 8; ++m) {
            const float v = acc[8 * half + (m & 3) + 4 * (m >> 2)] + bc;
            const bool take = v > best || (v != v && best == best);        // the first member on an exact tie; a NaN goes through
            best = take ? v : best;
            wb = take ? (unsigned)m : wb;
        }
        const int gb = G / ep3, gp = G - gb * ep3;
        out[((int64_t)gb * VX_C + r) * ep3 + gp] = best;                       // voxnet.py:23: the flatten order c Ep^3 + p
        win[(int64_t)G * VX_C + r] = (unsigned char)wb;
    }
}

// ---- backward: the pooled gradient channel-last, db2 --------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_T) void vox_gp_kernel(const float *__restrict__ gout, int ep3, int64_t n, float *__restrict__ gp)
{
    const int64_t i = (int64_t)blockIdx.x * VX_T + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i & 31);
    const int64_t G = i >> 5, b = G / ep3, p = G - b * ep3;
    gp[i] = gout[(b * VX_C + c) * ep3 + p];
}

// workgroup = channel: thread t sums groups t, t + 256, ... in order, the threads are added in thread order
__global__ __launch_bounds__(VX_T) void vox_db2_kernel(const float *__restrict__ gp, int NG, int accumulate, float *__restrict__ db)
{
    __shared__ float red[VX_T];
    const int c = blockIdx.x;
    float s = 0.f;
    for (int G = threadIdx.x; G < NG; G += VX_T) s += gp[(int64_t)G * VX_C + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int t = 1; t < VX_T; ++t) s += red[t];
    db[c] = accumulate ? db[c] + s : s;
}

// ---- conv2 backward: dX ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_T) void vox_conv2_dx_kernel(const float *__restrict__ gp, const unsigned char *__restrict__ win, const float *__restrict__ wt,
                                                           const float *__restrict__ y1, const float *__restrict__ mean, const float *__restrict__ invstd,
                                                           const float *__restrict__ scale, const float *__restrict__ shift, VxGeo g,
                                                           float *__restrict__ dz, float *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int m0 = (blockIdx.x * 4 + wv) * 32, m = m0 + r;
    const bool live = m < g.M1;
    const int e1 = g.E1, e13 = e1 * e1 * e1, ep3 = g.Ep * g.Ep * g.Ep, mc = live ? m : 0;
    const int b = mc / e13, p = mc - b * e13, z = p / (e1 * e1), yy = (p / e1) % e1, xx = p % e1;
    const float *wr = wt + r * (VX_C * VX_K2) + 8 * h;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int tz = 0; tz < 3; ++tz)
        for (int ty = 0; ty < 3; ++ty)
            for (int tx = 0; tx < 3; ++tx) {
                const int qz = z - tz, qy = yy - ty, qx = xx - tx;
                const bool vq = live && qz >= 0 && qz < g.E2 && qy >= 0 && qy < g.E2 && qx >= 0 && qx < g.E2;      // else: the zero halo
                const int tap = (tz * 3 + ty) * 3 + tx;
                const int G = vq ? b * ep3 + ((qz >> 1) * g.Ep + (qy >> 1)) * g.Ep + (qx >> 1) : 0;               // (the halo reads group 0 and selects nothing)
                const unsigned e = vq ? (unsigned)((qz & 1) * 4 + (qy & 1) * 2 + (qx & 1)) : 8u;
                const int64_t at = (int64_t)G * VX_C + 8 * h;
                // (straight-line: no branch around the MFMAs, neither per lane nor per wave)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    float av[8], bv[8];
                    vox_ld8(wr + tap * VX_C + 16 * q, bv);
                    vox_ld8(gp + at + 16 * q, av);
                    const uint2 wb = *reinterpret_cast<const uint2 *>(win + at + 16 * q);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const unsigned wj = ((j < 4 ? wb.x : wb.y) >> (8 * (j & 3))) & 0xffu;
                        av[j] = wj == e ? av[j] : 0.f;
                    }
                    acc = vox_step(av, bv, acc);
                }
            }
    vox_mfma_drain(acc);
    const float sc = scale[r], sh = shift[r], mu = mean[r], is = invstd[r];
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int mm = m0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (mm < g.M1) {
            const float yv = y1[(int64_t)mm * VX_C + r];
            const float d = fmaf(sc, yv, sh) > 0.f ? acc[i] : VX_SLOPE * acc[i];
            dz[(int64_t)mm * VX_C + r] = d;
            s += d;
            q = fmaf(d, (yv - mu) * is, q);
        }
    }
    vox_block_sums(s, q, part);
}

// ---- conv2 backward: dW ---------------------------------------------------------------------------------------------------------------------
// wave = tap (4 blockIdx.y + wave), chunk t (blockIdx.x) = pool groups VX_DWG t .. + VX_DWG - 1.  A[row r = co][k] = dY of member j of group
// G = g0 + 2 s + h, B[k][col r = ci] = a1 at that member's position + tap.  part + t * VX_W2N in the source's order (co 32 + ci) 27 + tap.
__global__ __launch_bounds__(VX_T) void vox_conv2_dw_kernel(const float *__restrict__ gp, const unsigned char *__restrict__ win, const float *__restrict__ y1,
                                                           const float *__restrict__ scale, const float *__restrict__ shift, VxGeo g, float *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int tap = blockIdx.y * 4 + wv;
    if (tap >= VX_K2) return;                                       // (wave-uniform; no barrier below)
    const int tz = tap / 9, ty = (tap / 3) % 3, tx = tap % 3;
    const int e1 = g.E1, ep3 = g.Ep * g.Ep * g.Ep;
    const int g0 = blockIdx.x * VX_DWG, g1 = min(g0 + VX_DWG, g.NG);
    const float sc = scale[r], sh = shift[r];
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int gs = g0; gs < g1; gs += 2) {
        const int G = gs + h;
        const bool in = G < g1;
        const int Gc = in ? G : g0;
        const int b = Gc / ep3, p = Gc - b * ep3, pz = p / (g.Ep * g.Ep), py = (p / g.Ep) % g.Ep, px = p % g.Ep;
        const int row0 = ((b * e1 + 2 * pz + tz) * e1 + 2 * py + ty) * e1 + 2 * px + tx;
        const float gv = in ? gp[(int64_t)Gc * VX_C + r] : 0.f;
        const unsigned wb = win[(int64_t)Gc * VX_C + r];
        float av[8], bv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            av[j] = wb == (unsigned)j ? gv : 0.f;
            const int ro = row0 + ((j >> 2) * e1 + ((j >> 1) & 1)) * e1 + (j & 1);
            const float a1 = vox_leaky(fmaf(sc, y1[(int64_t)ro * VX_C + r], sh));      // (always loaded: a padding group reads group g0)
            bv[j] = in ? a1 : 0.f;
        }
        acc = vox_step(av, bv, acc);
    }
    vox_mfma_drain(acc);
    float *pt = part + (int64_t)blockIdx.x * VX_W2N;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int co = (i & 3) + 8 * (i >> 2) + 4 * h;
        pt[(co * VX_C + r) * VX_K2 + tap] = acc[i];
    }
}

// ---- conv1 backward: dW ---------------------------------------------------------------------------------------------------------------------
// wave = taps 32 wave .. + 31, chunk t (blockIdx.x) = rows VX_W1CH t .. of y1.  A[row r = co][k = row] = dy1 = scale (dz - c1 - xhat c2),
// B[k = row][col r = tap] = the input under that tap.  part + t * 32 * 125 in the source's order co 125 + tap.
__global__ __launch_bounds__(VX_T) void vox_conv1_dw_kernel(const float *__restrict__ dz, const float *__restrict__ y1, const float *__restrict__ mean,
                                                           const float *__restrict__ invstd, const float *__restrict__ scale, const float *__restrict__ c1,
                                                           const float *__restrict__ c2, const float *__restrict__ x, VxGeo g, float *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int tap = 32 * wv + r;
    const bool tin = tap < VX_K1;
    const int tc = tin ? tap : 0;
    const int E = g.E, e1 = g.E1, e13 = e1 * e1 * e1;
    const int to = ((tc / 25) * E + (tc / 5) % 5) * E + tc % 5;
    const float mu = mean[r], is = invstd[r], sc = scale[r], k1 = c1[r], k2 = c2[r];
    const int r0 = blockIdx.x * VX_W1CH;
    floatx16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int nks = min(VX_W1CH / 16, (g.M1 - r0 + 15) / 16);
    for (int ks = 0; ks < nks; ++ks) {
        const int mb = r0 + ks * 16 + 8 * h;
        float av[8], bv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = mb + j;
            const bool in = m < g.M1;
            const int mc = in ? m : 0;
            const int b = mc / e13, p = mc - b * e13, z = p / (e1 * e1), yy = (p / e1) % e1, xx = p % e1;
            const float yv = y1[(int64_t)mc * VX_C + r], d = dz[(int64_t)mc * VX_C + r];
            const float xv = x[(int64_t)b * E * E * E + ((2 * z) * E + 2 * yy) * E + 2 * xx + to];      // (always loaded: row 0 / tap 0 stand in)
            av[j] = in ? sc * ((d - k1) - ((yv - mu) * is) * k2) : 0.f;
            bv[j] = (in && tin) ? xv : 0.f;
        }
        acc = vox_step(av, bv, acc);
    }
    vox_mfma_drain(acc);
    if (!tin) return;
    float *pt = part + (int64_t)blockIdx.x * (VX_C * VX_K1);
#pragma unroll
    for (int i = 0; i < 16; ++i) pt[((i & 3) + 8 * (i >> 2) + 4 * h) * VX_K1 + tap] = acc[i];
}

__global__ __launch_bounds__(64) void vox_zero_kernel(float *__restrict__ p, int n)
{
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0.f;
}

// ---- the head's LeakyReLU + dropout (upscale in train) --------------------------------------------------------------------------------------
__global__ __launch_bounds__(VX_T) void vox_leaky_drop_fwd_kernel(const float *__restrict__ x, int64_t n, float slope, float drop_p,
                                                                 const int64_t *__restrict__ rng_state, int tag, float *__restrict__ out,
                                                                 unsigned char *__restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * VX_T + threadIdx.x;
    if (i >= n) return;
    const bool drop = rng_state != nullptr && drop_p > 0.f;
    const float v = x[i], a = v > 0.f ? v : slope * v;
    bool k = true;
    if (drop) k = hash_uniform((uint64_t)rng_state[0], (uint64_t)rng_state[1], (uint32_t)tag, (uint32_t)i) >= drop_p;
    if (keep) keep[i] = k ? 1 : 0;
    out[i] = k ? a * (drop ? 1.0f / (1.0f - drop_p) : 1.0f) : 0.f;
}

// (a launch of its own behind the mask draw: every thread of the draw has read the counter)
__global__ __launch_bounds__(64) void vox_rng_bump_kernel(int64_t *rng_state)
{
    if (threadIdx.x == 0) rng_state[1] += 1;
}

__global__ __launch_bounds__(VX_T) void vox_leaky_drop_bwd_kernel(const float *__restrict__ gout, const float *__restrict__ x, const unsigned char *__restrict__ keep,
                                                                 int64_t n, float slope, float drop_p, float *__restrict__ dx)
{
    const int64_t i = (int64_t)blockIdx.x * VX_T + threadIdx.x;
    if (i >= n) return;
    const bool k = keep ? keep[i] != 0 : true;
    const float gs = gout[i] * (keep && drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f);
    dx[i] = k ? (x[i] > 0.f ? gs : slope * gs) : 0.f;
}

// ---- occupancy grid -----------------------------------------------------------------------------------------------------------------------------
// build_VoxData.py:58-60: arr[int(x 15.5 + 15.5)][int(y 15.5 + 15.5)][int(z 15.5 + 15.5)] = 1, (E - 1) / 2 for 15.5; the index in double from the
// exactly widened fp32 coordinate, product and sum rounded separately (numpy's evaluation).  Outside [-1, 1] (or NaN): clamped and counted.
__global__ __launch_bounds__(VX_T) void vox_occupancy_kernel(const float *__restrict__ pts, int64_t n_pts, int N, int E, float *__restrict__ grid,
                                                            unsigned *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * VX_T + threadIdx.x;
    if (i >= n_pts) return;
    const double half = (double)(E - 1) * 0.5;
    int idx[3];
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float c = pts[3 * i + a];
        if (!(c >= -1.f && c <= 1.f)) bad = true;
        const double d = __dadd_rn(__dmul_rn((double)c, half), half);
        int v = d >= 0.0 ? (d < (double)E ? (int)d : E - 1) : 0;     // (a NaN lands in 0)
        idx[a] = v;
    }
    if (bad) atomicAdd(err, 1u);
    grid[(i / N) * (int64_t)E * E * E + ((int64_t)idx[0] * E + idx[1]) * E + idx[2]] = 1.0f;
}

__global__ __launch_bounds__(VX_T) void vox_fill0_kernel(float *__restrict__ p, int64_t n, unsigned *__restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * VX_T + threadIdx.x;
    if (i == 0 && err) *err = 0u;
    if (i < n) p[i] = 0.f;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------
static bool vox_ok(int E)
{
    if (E < 5 || E > 32) return false;
    const int E1 = (E - 5) / 2 + 1, E2 = E1 - 2;
    return E1 >= 3 && E2 >= 2 && E2 % 2 == 0;
}

static int vox_geo(const char *who, int B, int E, VxGeo &g)
{
    PAPC_REQUIRE(vox_ok(E), PAPC_E_UNSUPPORTED, "%s: E=%d (input edge: at most 32, conv1 edge (E - 5) / 2 + 1 >= 3, conv2 edge even)", who, E);
    PAPC_REQUIRE(B >= 1 && B <= 4096, PAPC_E_INVALID, "%s: B=%d (1 .. 4096 clouds)", who, B);
    g.B = B; g.E = E; g.E1 = (E - 5) / 2 + 1; g.E2 = g.E1 - 2; g.Ep = g.E2 / 2;
    g.M1 = B * g.E1 * g.E1 * g.E1;
    g.NG = B * g.Ep * g.Ep * g.Ep;
    return PAPC_OK;
}

static size_t vox_pad4(size_t n) { return (n + 3) & ~(size_t)3; }

}  // namespace papc

using namespace papc;

extern "C" {

int papc_voxconv_ok(int E) { return vox_ok(E) ? 1 : 0; }

int papc_voxconv_parts(int B, int E)
{
    VxGeo g;
    if (B < 1 || B > 4096 || !vox_ok(E)) return 0;
    vox_geo("papc_voxconv_parts", B, E, g);
    return (int)cdiv(g.M1, 128);
}

int papc_voxconv1_fwd_f32(const float *x, const float *w1, const float *b1, int B, int E, float *y1, float *stats_partial, papc_stream_t stream)
{
    const char *who = "papc_voxconv1_fwd_f32";
    VxGeo g;
    const int err = vox_geo(who, B, E, g);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(x && w1 && y1 && stats_partial, PAPC_E_INVALID, "%s: null pointer", who);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MLP_GEMM, st);
    hipLaunchKernelGGL(vox_conv1_fwd_kernel, dim3((unsigned)cdiv(g.M1, 128)), dim3(VX_T), 0, st, x, w1, b1, g, y1, stats_partial);
    return check_launch(who);
}

int papc_voxconv2_prep_f32(const float *w2, float *wk, float *wt, papc_stream_t stream)
{
    PAPC_REQUIRE(w2 && wk && wt && aligned16(wk) && aligned16(wt), PAPC_E_INVALID, "papc_voxconv2_prep_f32: null or misaligned pointer");
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(vox_w2_prep_kernel, dim3((unsigned)cdiv(VX_W2N, VX_T)), dim3(VX_T), 0, st, w2, wk, wt);
    return check_launch("papc_voxconv2_prep_f32");
}

int papc_voxconv2_pool_fwd_f32(const float *y1, const float *scale, const float *shift, const float *wk, const float *b2, int B, int E, float *out,
                               uint8_t *win, papc_stream_t stream)
{
    const char *who = "papc_voxconv2_pool_fwd_f32";
    VxGeo g;
    const int err = vox_geo(who, B, E, g);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(y1 && scale && shift && wk && out && win, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(aligned16(y1) && aligned16(scale) && aligned16(shift) && aligned16(wk), PAPC_E_INVALID, "%s: y1, scale, shift and wk must be 16-byte aligned", who);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MLP_GEMM, st);
    hipLaunchKernelGGL(vox_conv2_pool_kernel, dim3((unsigned)cdiv(g.NG, 16)), dim3(VX_T), 0, st, y1, scale, shift, wk, b2, g, out, win);
    return check_launch(who);
}

int papc_voxconv2_bwd_dx_f32(const float *gout, const uint8_t *win, const float *wt, const float *y1, const float *mean, const float *invstd,
                             const float *scale, const float *shift, int B, int E, float *gp, float *dz, float *red_partial, papc_stream_t stream)
{
    const char *who = "papc_voxconv2_bwd_dx_f32";
    VxGeo g;
    const int err = vox_geo(who, B, E, g);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(gout && win && wt && y1 && mean && invstd && scale && shift && gp && dz && red_partial, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(aligned16(gp) && aligned16(wt) && (reinterpret_cast<uintptr_t>(win) & 7) == 0, PAPC_E_INVALID,
                 "%s: gp and wt must be 16-byte aligned, the winner bytes 8-byte aligned", who);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_BWD_DX, st);
    const int64_t n = (int64_t)g.NG * VX_C;
    hipLaunchKernelGGL(vox_gp_kernel, dim3((unsigned)cdiv(n, VX_T)), dim3(VX_T), 0, st, gout, g.Ep * g.Ep * g.Ep, n, gp);
    hipLaunchKernelGGL(vox_conv2_dx_kernel, dim3((unsigned)cdiv(g.M1, 128)), dim3(VX_T), 0, st, gp, win, wt, y1, mean, invstd, scale, shift, g, dz, red_partial);
    return check_launch(who);
}

size_t papc_voxconv2_bwd_dw_workspace(int B, int E)
{
    VxGeo g;
    if (B < 1 || B > 4096 || !vox_ok(E)) return 0;
    vox_geo("papc_voxconv2_bwd_dw_workspace", B, E, g);
    return (size_t)cdiv(g.NG, VX_DWG) * VX_W2N * sizeof(float);
}

int papc_voxconv2_bwd_dw_f32(const float *gp, const uint8_t *win, const float *y1, const float *scale, const float *shift, int B, int E, float *dw2,
                             float *db2, int accumulate, void *workspace, size_t workspace_bytes, papc_stream_t stream)
{
    const char *who = "papc_voxconv2_bwd_dw_f32";
    VxGeo g;
    const int err = vox_geo(who, B, E, g);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(gp && win && y1 && scale && shift && dw2 && workspace, PAPC_E_INVALID, "%s: null pointer", who);
    const size_t need = papc_voxconv2_bwd_dw_workspace(B, E);
    PAPC_REQUIRE(workspace_bytes >= need && aligned16(workspace), PAPC_E_INVALID, "%s: workspace %zu bytes < %zu (or not 16-byte aligned)", who, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const int T = (int)cdiv(g.NG, VX_DWG);
    float *part = static_cast<float *>(workspace);
    {
        ProfScope prof(PAPC_K_BWD_DW, st);
        hipLaunchKernelGGL(vox_conv2_dw_kernel, dim3((unsigned)T, (unsigned)cdiv(VX_K2, 4)), dim3(VX_T), 0, st, gp, win, y1, scale, shift, g, part);
        if (db2) hipLaunchKernelGGL(vox_db2_kernel, dim3(VX_C), dim3(VX_T), 0, st, gp, g.NG, accumulate, db2);
        const int e = check_launch(who);
        if (e != PAPC_OK) return e;
    }
    return papc_reduce_partials_f32(part, T, VX_W2N, dw2, accumulate, stream);             // the chunks in chunk order (fold.h)
}

size_t papc_voxconv1_bwd_dw_workspace(int B, int E)
{
    VxGeo g;
    if (B < 1 || B > 4096 || !vox_ok(E)) return 0;
    vox_geo("papc_voxconv1_bwd_dw_workspace", B, E, g);
    return vox_pad4((size_t)cdiv(g.M1, VX_W1CH) * VX_C * VX_K1) * sizeof(float);
}

int papc_voxconv1_bwd_dw_f32(const float *dz, const float *y1, const float *mean, const float *invstd, const float *scale, const float *c1, const float *c2,
                             const float *x, int B, int E, float *dw1, float *db1, int accumulate, void *workspace, size_t workspace_bytes,
                             papc_stream_t stream)
{
    const char *who = "papc_voxconv1_bwd_dw_f32";
    VxGeo g;
    const int err = vox_geo(who, B, E, g);
    if (err != PAPC_OK) return err;
    PAPC_REQUIRE(dz && y1 && mean && invstd && scale && c1 && c2 && x && dw1 && workspace, PAPC_E_INVALID, "%s: null pointer", who);
    const size_t need = papc_voxconv1_bwd_dw_workspace(B, E);
    PAPC_REQUIRE(workspace_bytes >= need && aligned16(workspace), PAPC_E_INVALID, "%s: workspace %zu bytes < %zu (or not 16-byte aligned)", who, workspace_bytes, need);
    hipStream_t st = as_stream(stream);
    const int T = (int)cdiv(g.M1, VX_W1CH);
    float *part = static_cast<float *>(workspace);
    {
        ProfScope prof(PAPC_K_BWD_DW, st);
        hipLaunchKernelGGL(vox_conv1_dw_kernel, dim3((unsigned)T), dim3(VX_T), 0, st, dz, y1, mean, invstd, scale, c1, c2, x, g, part);
        if (db1 && !accumulate) hipLaunchKernelGGL(vox_zero_kernel, dim3(1), dim3(64), 0, st, db1, VX_C);    // a bias under a train-mode norm: exactly 0
        const int e = check_launch(who);
        if (e != PAPC_OK) return e;
    }
    return papc_reduce_partials_f32(part, T, VX_C * VX_K1, dw1, accumulate, stream);        // the chunks in chunk order (fold.h)
}

int papc_leaky_dropout_fwd_f32(const float *x, int64_t n, float slope, float drop_p, int64_t *rng_state, int tag, int bump, float *out, uint8_t *keep,
                               papc_stream_t stream)
{
    const char *who = "papc_leaky_dropout_fwd_f32";
    PAPC_REQUIRE(x && out, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), PAPC_E_INVALID, "%s: n=%lld", who, (long long)n);
    PAPC_REQUIRE(drop_p >= 0.f && drop_p < 1.f, PAPC_E_INVALID, "%s: drop_p=%f", who, (double)drop_p);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(vox_leaky_drop_fwd_kernel, dim3((unsigned)cdiv(n, VX_T)), dim3(VX_T), 0, st, x, n, slope, drop_p, rng_state, tag, out, keep);
    if (bump && rng_state && drop_p > 0.f) hipLaunchKernelGGL(vox_rng_bump_kernel, dim3(1), dim3(64), 0, st, rng_state);
    return check_launch(who);
}

int papc_leaky_dropout_bwd_f32(const float *gout, const float *x, const uint8_t *keep, int64_t n, float slope, float drop_p, float *dx, papc_stream_t stream)
{
    const char *who = "papc_leaky_dropout_bwd_f32";
    PAPC_REQUIRE(gout && x && dx, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), PAPC_E_INVALID, "%s: n=%lld", who, (long long)n);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(vox_leaky_drop_bwd_kernel, dim3((unsigned)cdiv(n, VX_T)), dim3(VX_T), 0, st, gout, x, keep, n, slope, drop_p, dx);
    return check_launch(who);
}

int papc_occupancy_grid_f32(const float *points, int B, int N, int E, float *grid, uint32_t *err, papc_stream_t stream)
{
    const char *who = "papc_occupancy_grid_f32";
    PAPC_REQUIRE(points && grid && err, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(B >= 1 && N >= 1 && E >= 1 && E <= 1024 && (int64_t)B * N < ((int64_t)1 << 31) && (int64_t)B * E * E * E < ((int64_t)1 << 40), PAPC_E_INVALID,
                 "%s: B=%d N=%d E=%d", who, B, N, E);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    const int64_t n = (int64_t)B * E * E * E;
    hipLaunchKernelGGL(vox_fill0_kernel, dim3((unsigned)cdiv(n, VX_T)), dim3(VX_T), 0, st, grid, n, err);
    hipLaunchKernelGGL(vox_occupancy_kernel, dim3((unsigned)cdiv((int64_t)B * N, VX_T)), dim3(VX_T), 0, st, points, (int64_t)B * N, N, E, grid, err);
    return check_launch(who);
}

}  // extern "C"
