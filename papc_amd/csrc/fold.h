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
// QUARTER FOLD  fold_quarters_f64: a wave owns 16 elements; lane & 15 = element, lane >> 4 = quarter q of the chunks,
//   [q * per, min(n_chunks, (q + 1) * per)) with per = ceil(n_chunks / 4).  In float64:
//     s_q = 0.0;  s_q += part[t] for the quarter's t in order;      total = ((s_0 + s_1) + s_2) + s_3
//   (eight loads in flight, the sum does not depend on it)
//     dw_max_fold_kernel (mlp_dw.hip) and fold_jobs_kernel's PAPC_FOLD_F64Q kind (folds.hip): a deferred fold has that launch's bits
//
// What a fold does with its total is the caller's: `accumulate` adds it to what the output held, as the last add.
#pragma once
#include "common.h"

namespace papc {

// ---- host: the entries of a papc_fold_list beyond the float fold (include/papc_hip.h) -----------------------------------------------------
static inline bool fold_list_room(const papc_fold_list *fl, int slots) { return fl && fl->jobs && fl->count + slots <= fl->capacity; }
static inline void fold_list_push_f64q(papc_fold_list *fl, const float *partial, int n_chunks, int64_t ld, int n, double *out)
{
    papc_fold_job &j = fl->jobs[fl->count++];
    memset(&j, 0, sizeof(j));
    j.partial = partial; j.n_chunks = n_chunks; j.ld = ld; j.rows = PAPC_FOLD_F64Q; j.cols = n; j.out = reinterpret_cast<float *>(out); j.out_ld = n;
}
static inline void fold_list_push_fin(papc_fold_list *fl, const papc_fold_fin &f)
{
    papc_fold_job &j = fl->jobs[fl->count];
    memset(&j, 0, sizeof(j) * (1 + PAPC_FOLD_FIN_SLOTS));
    j.rows = PAPC_FOLD_FIN; j.n_chunks = PAPC_FOLD_FIN_SLOTS; j.cols = f.kind;
    memcpy(&fl->jobs[fl->count + 1], &f, sizeof(f));
    fl->count += 1 + PAPC_FOLD_FIN_SLOTS;
}

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

// The quarter fold of element e (every lane of a wave calls; `live` = this lane's element exists).  True on the one lane per element that
// holds the total.
__device__ __forceinline__ bool fold_quarters_f64(const float *__restrict__ part, int64_t ld, int n_chunks, int64_t e, bool live, double &total)
{
    const int l = threadIdx.x & 15, q = (threadIdx.x & 63) >> 4;
    const int per = (n_chunks + 3) / 4, c0 = q * per, c1 = min(n_chunks, c0 + per);
    double s = 0.0;
    if (live) {
        int c = c0;
        for (; c + 8 <= c1; c += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = part[(int64_t)(c + j) * ld + e];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += (double)v[j];
        }
        for (; c < c1; ++c) s += (double)part[(int64_t)c * ld + e];
    }
    const double s1 = __shfl(s, l + 16), s2 = __shfl(s, l + 32), s3 = __shfl(s, l + 48);
    total = ((s + s1) + s2) + s3;
    return q == 0 && live;
}

}  // namespace papc
