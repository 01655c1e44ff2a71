// fold.h -- the summation orders of the partial-sum folds, written once.
//
// Every backward kernel writes per-workgroup (per-chunk) partial sums and a fold adds them up.  The ORDER of that sum is a contract: a
// training step is bit-reproducible, and the launch-structure tests compare two paths bit for bit -- two folds that may stand in for
// each other (a stack's own launch and the step's deferred fold, a fused tail and the two launches it replaces) must add the same
// numbers in the same order.  This comment is the only place the orders are specified; tests/test_gpu_fold_order.py pins them against
// a float32 emulation.  part[t * ld + i] is element i of chunk t, t < n_chunks; an element is a float or a float4 of four of them.
//
// LANE FOLD  fold_lanes<FW, NLOAD>: a workgroup of FW waves owns 64 elements; lane = element (coalesced), wave = chunk lane cl.
//     s_cl = 0.f;  s_cl += part[t] for t = cl, cl + FW, cl + 2 FW, ... in that order;      total = s_0;  total += s_g for g = 1 .. FW - 1
//   NLOAD loads are in flight per lane; the sum does not depend on NLOAD.  A load past the last chunk re-reads chunk t0 and is left out
//   of the sum -- a float lane adds 0.f in its place, which leaves the same bits: a sum that started from 0.f is never -0.0.
//   A lane without a chunk (n_chunks < FW) contributes its 0.f.
//     FW = 16, NLOAD = 8    reduce_partials_kernel, reduce_partials_batch_kernel (folds.hip)
//     FW = 16, NLOAD = 32   pfn_bwd_fold_finalize_kernel (pfn.hip)
//     FW = 4, float4        reduce_partials_wide_kernel (folds.hip), NLOAD = 4
//     FW = PAPC_FOLD_WAVES  fold_jobs_kernel's many-chunk shapes, float and float4 (folds.hip), NLOAD = 8: at the default of 16 a
//                           deferred fold has the bits of reduce_partials_batch_kernel
//
// IN-ORDER FOLD  fold_in_order<NLOAD, START>: one thread owns an element and walks the chunks 0, 1, 2, ...
//     FOLD_FROM_FIRST:  s = part[0];         s += part[t] for t = 1, 2, ...       (a single chunk is copied: -0.0 stays -0.0)
//     FOLD_FROM_ZERO:   s = 0.f;             s += part[t] for t = 0, 1, 2, ...
//   NLOAD loads in flight, the sum does not depend on it; a load past the last chunk is left out (nothing is added in its place).
//     FOLD_FROM_FIRST   fold_jobs_kernel's few-chunk (wide) shape (folds.hip, NLOAD = 8), pg_fold_kernel (smallm.hip),
//                       ct_fold_kernel (cloud_transform.hip)
//     FOLD_FROM_ZERO    cc_fold_kernel (cloud_concat.hip): NLOAD = 4 for the weight block; cc_fold_s (cloud_concat.h, the per-cloud sums of
//                       cc_fold_kernel and cck_fold_kernel): NLOAD = 1
//
// SLICE TREE  reduce_partials_strided_kernel (folds.hip), its only user: 64 slices, slice sl sums chunks sl, sl + 64, ... to 0.f in
//   order (a missing chunk adds 0.f), then red[sl] += red[sl + h] for h = 32, 16, ... 1.
//
// What a fold does with its total is the caller's: `accumulate` adds it to what the output held, as the last add.
#pragma once
#include "common.h"

namespace papc {

template <typename V> __device__ __forceinline__ V fold_zero();
template <> __device__ __forceinline__ float fold_zero<float>() { return 0.f; }
template <> __device__ __forceinline__ float4 fold_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float fold_add(float s, float v) { return s + v; }
__device__ __forceinline__ float4 fold_add(float4 s, const float4 &v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; return s; }
// (lane fold only: s never holds -0.0 there)
__device__ __forceinline__ float fold_add_if(float s, float v, bool take) { return s + (take ? v : 0.f); }
__device__ __forceinline__ float4 fold_add_if(float4 s, const float4 &v, bool take) { return take ? fold_add(s, v) : s; }

// The lane fold of element(s) i of a workgroup of 64 * FW threads (every thread calls; `live` = this lane's element exists).  True on
// the one lane per element that holds the total.
template <int FW, int NLOAD, typename V>
__device__ __forceinline__ bool fold_lanes(const float *__restrict__ part, int64_t ld, int n_chunks, int64_t i, bool live, V (&red)[FW][64], V &total)
{
    const int el = threadIdx.x & 63, cl = threadIdx.x >> 6;
    V s = fold_zero<V>();
    if (live) {
        for (int t0 = cl; t0 < n_chunks; t0 += FW * NLOAD) {
            V v[NLOAD];
#pragma unroll
            for (int j = 0; j < NLOAD; ++j) {
                const int t = t0 + FW * j;
                v[j] = *reinterpret_cast<const V *>(part + (int64_t)(t < n_chunks ? t : t0) * ld + i);
            }
#pragma unroll
            for (int j = 0; j < NLOAD; ++j) s = fold_add_if(s, v[j], t0 + FW * j < n_chunks);
        }
    }
    red[cl][el] = s;
    __syncthreads();
    const bool top = cl == 0 && live;
    if (top) {
#pragma unroll
        for (int g = 1; g < FW; ++g) s = fold_add(s, red[g][el]);
    }
    total = s;
    return top;
}

enum FoldStart { FOLD_FROM_FIRST, FOLD_FROM_ZERO };

// The in-order fold of element(s) i.
template <int NLOAD, FoldStart START, typename V>
__device__ __forceinline__ V fold_in_order(const float *__restrict__ part, int64_t ld, int n_chunks, int64_t i)
{
    V s = fold_zero<V>();
    for (int t0 = 0; t0 < n_chunks; t0 += NLOAD) {
        V v[NLOAD];
#pragma unroll
        for (int j = 0; j < NLOAD; ++j) v[j] = *reinterpret_cast<const V *>(part + (int64_t)(t0 + j < n_chunks ? t0 + j : t0) * ld + i);
#pragma unroll
        for (int j = 0; j < NLOAD; ++j)
            if (t0 + j < n_chunks) { if (START == FOLD_FROM_FIRST && t0 + j == 0) s = v[j]; else s = fold_add(s, v[j]); }
    }
    return s;
}

}  // namespace papc
