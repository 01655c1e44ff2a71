// kdsel.h -- the kd-tree select's index rule, written once for kdconv.hip (KD-Net levels) and kdbn.hip (KDUNet down levels).
//
// For pre-pool row n of a cloud, s = sel[n] in {0, 1, 2}:  j = 3n + s,  k = j / dim (weight plane),  p = j % dim (source point): the source's
// two reshapes and its index arithmetic as they are (kdnet.py:21-30, kdunet.py:51-61).
#pragma once
#include "common.h"

namespace papc {

constexpr unsigned KD_ROW = 0x3fffffffu;

__device__ __forceinline__ float4 kd_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ int kd_clamp_s(int s) { return min(max(s, 0), 2); }

// pre-pool row m of the flattened rows -> (plane k << 30) | flattened source row; k = 3 for a row past M.  A split value outside 0..2 is
// clamped, so it cannot address outside the buffers.
__device__ __forceinline__ unsigned kd_row_info(int m, int M, int dim, const int *__restrict__ sel, int64_t ss)
{
    if (m >= M) return 3u << 30;
    const int b = m / dim, n = m - b * dim;
    const int j = 3 * n + kd_clamp_s(sel[(int64_t)b * ss + n]);
    const int k = (j >= dim) + (j >= 2 * dim);
    return ((unsigned)k << 30) | (unsigned)(b * dim + j - k * dim);
}

// the row of cloud b that source point p feeds through plane q, if any: 3n + s = p + q dim with s = sel[n]
__device__ __forceinline__ bool kd_fed_row(int b, int p, int q, int dim, const int *__restrict__ sel, int64_t ss, int &n)
{
    const int t = p + q * dim;
    n = t / 3;
    return kd_clamp_s(sel[(int64_t)b * ss + n]) == t - 3 * n;
}

}  // namespace papc
