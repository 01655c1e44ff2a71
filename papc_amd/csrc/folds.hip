// folds.hip -- the generic folds of per-chunk partial sums (gfx950): out[i] (+)= sum_t partial[t, i] in a FIXED order, so that a training
// step is bit-reproducible.  The orders are specified in fold.h and nowhere else.  The folds that belong to one producer (pg_fold_kernel,
// ct_fold_kernel, cc_fold_kernel, the pfn tail, ...) live beside it and call into fold.h as well.
#include <vector>

#include "finalize.h"
#include "fold.h"

namespace papc {

// lane fold, FW = 16; elements [0, n1) -> out, [n1, n) -> out2
__device__ __forceinline__ void reduce_partials_body(float (&red)[16][64], const float *__restrict__ part, int n_chunks, int64_t n, int64_t ld,
                                                     float *__restrict__ out, int64_t n1, float *__restrict__ out2, int accumulate)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    float s;
    if (fold_lanes<16, 8>(part, ld, n_chunks, i, i < n, red, s)) {
        float *o = i < n1 ? out + i : out2 + (i - n1);
        *o = accumulate ? *o + s : s;
    }
}

__global__ __launch_bounds__(1024) void reduce_partials_kernel(const float *__restrict__ part, int n_chunks, int64_t n,
                                                               int64_t ld, float *__restrict__ out, int64_t n1,
                                                               float *__restrict__ out2, int accumulate)
{
    __shared__ float red[16][64];
    reduce_partials_body(red, part, n_chunks, n, ld, out, n1, out2, accumulate);
}

// up to 8 partial reductions in one launch (blockIdx.y = job): the dW partials of all layers of a stack are folded together at the end
// of its backward instead of one launch-latency-sized kernel per layer
struct ReduceBatch {
    const float *part[8]; float *out1[8], *out2[8];
    int64_t ld[8], n1[8], n[8];
    int n_chunks[8], accumulate[8];
};
__global__ __launch_bounds__(1024) void reduce_partials_batch_kernel(ReduceBatch b)
{
    __shared__ float red[16][64];
    const int job = blockIdx.y;
    if ((int64_t)blockIdx.x * 64 >= b.n[job]) return;               // (uniform per workgroup: this job is narrower than the widest one)
    reduce_partials_body(red, b.part[job], b.n_chunks[job], b.n[job], b.ld[job], b.out1[job], b.n1[job], b.out2[job], b.accumulate[job]);
}

// few chunks of many elements (the group_all layers): a lane owns 4 consecutive elements, the 4 waves of a workgroup are the chunk
// lanes; n1, ld multiples of 4 and 16-byte aligned pointers
__global__ __launch_bounds__(256) void reduce_partials_wide_kernel(const float *__restrict__ part, int n_chunks, int64_t n, int64_t ld,
                                                                   float *__restrict__ out, int64_t n1, float *__restrict__ out2,
                                                                   int accumulate)
{
    __shared__ float4 red[4][64];
    const int64_t i = ((int64_t)blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    float4 s;
    if (fold_lanes<4, 4>(part, ld, n_chunks, i, i < n, red, s)) {
        float4 *o = reinterpret_cast<float4 *>(i < n1 ? out + i : out2 + (i - n1));
        if (accumulate) s = fold_add(s, *o);
        *o = s;
    }
}

// out[r * out_ld + c] (+)= sum_t part[t * ld + r * cols + c]: the slice tree.  A workgroup = 16 consecutive elements x 64 chunk slices.
// (One thread per element walking all chunks took 80+ us for the 2048 x 192 gather-add partials.)
__global__ __launch_bounds__(1024) void reduce_partials_strided_kernel(const float *__restrict__ part, int n_chunks, int64_t ld, int rows, int cols,
                                                                       float *__restrict__ out, int64_t out_ld, int accumulate)
{
    __shared__ float red[64][17];
    const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int64_t n = (int64_t)rows * cols;
    const int64_t e = (int64_t)blockIdx.x * 16 + el;
    float s = 0.f;
    if (e < n) {
        for (int t0 = sl; t0 < n_chunks; t0 += 64 * 4) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (t0 + 64 * j < n_chunks) ? part[(int64_t)(t0 + 64 * j) * ld + e] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) s += v[j];
        }
    }
    red[sl][el] = s;
    __syncthreads();
    for (int h = 32; h >= 1; h >>= 1) {
        if (sl < h) red[sl][el] += red[sl + h][el];
        __syncthreads();
    }
    if (sl == 0 && e < n) {
        const int r = (int)(e / cols), c = (int)(e - (int64_t)r * cols);
        float *o = out + (int64_t)r * out_ld + c;
        *o = accumulate ? *o + red[0][el] : red[0][el];
    }
}

// ---- deferred folds: every partial reduction of a training step's backward in ONE launch (papc_fold_jobs_f32) ---------------------------
// Flat grid: workgroup b belongs to the job whose [wg0, wg0 + nwg) range holds it.  Three shapes, uniform per workgroup:
//   many chunks:          the lane fold, 64 elements per workgroup;
//   many chunks, float4:  the lane fold of 64 float4 (n % 4 == 0, contiguous output): 1 KB per wave and chunk;
//   few chunks (wide):    the in-order fold from the first chunk, a thread owns a float4 of 4 * 64 * FW consecutive elements per workgroup:
//                         the split-K partials of the planes path (<= 8 chunks of up to 512 K elements).
// and one more kind: the float64 quarter fold (PAPC_FOLD_F64Q), 16 elements per wave -- the no-store max layer's dW sums, which its
// closed form reads in the finalize launch below.
struct FoldBatch {
    const float *part[PAPC_FOLD_MAX]; float *out[PAPC_FOLD_MAX];
    int64_t ld[PAPC_FOLD_MAX], out_ld[PAPC_FOLD_MAX];
    int n_chunks[PAPC_FOLD_MAX], rows[PAPC_FOLD_MAX], cols[PAPC_FOLD_MAX], wg0[PAPC_FOLD_MAX + 1];
    unsigned acc_mask, wide_mask, vec_mask, f64_mask;
    int count;
};
// FW = chunk lanes (waves) per workgroup (PAPC_FOLD_WAVES).  Round 6 tried 8 instead of 16 -- the step's 654 workgroups of 1024 threads are two
// residency rounds (512 fit the chip), the second a quarter full; at 512 threads all are resident at once -- and measured it 7 us SLOWER per step
// (1.461 against 1.454 ms, same box, fixed plan): 16 stays the default.
template <int FW>
__global__ __launch_bounds__(64 * FW) void fold_jobs_kernel(FoldBatch b)
{
    __shared__ float red[FW][64];
    int job = 0;
    while (job + 1 < b.count && (int)blockIdx.x >= b.wg0[job + 1]) ++job;       // (<= 24 scalar compares)
    const int wg = (int)blockIdx.x - b.wg0[job];
    const float *__restrict__ part = b.part[job];
    float *__restrict__ out = b.out[job];
    const int64_t ld = b.ld[job], out_ld = b.out_ld[job];
    const int n_chunks = b.n_chunks[job], cols = b.cols[job];
    const int64_t n = (int64_t)b.rows[job] * cols;
    const bool acc = (b.acc_mask >> job) & 1u;
    if ((b.f64_mask >> job) & 1u) {         // PAPC_FOLD_F64Q: the quarter fold into a double output, a wave owns 16 elements
        const int64_t e = ((int64_t)wg * FW + (threadIdx.x >> 6)) * 16 + (threadIdx.x & 15);
        double t;
        if (fold_quarters_f64(part, ld, n_chunks, e, e < n, t)) reinterpret_cast<double *>(out)[e] = t;
        return;
    }
    if ((b.wide_mask >> job) & 1u) {       // few chunks, contiguous output (out_ld == cols), n % 4 == 0, 16-byte aligned
        const int64_t e = ((int64_t)wg * (64 * FW) + threadIdx.x) * 4;
        if (e >= n) return;
        float4 s = fold_in_order<8, FOLD_FROM_FIRST, float4>(part, ld, n_chunks, e);
        float4 *o = reinterpret_cast<float4 *>(out + e);
        if (acc) s = fold_add(s, *o);
        *o = s;
        return;
    }
    const int el = threadIdx.x & 63;
    if ((b.vec_mask >> job) & 1u) {         // many chunks, float4 lanes (n % 4 == 0, contiguous output)
        __shared__ float4 red4[FW][64];
        const int64_t i4 = ((int64_t)wg * 64 + el) * 4;
        float4 s4;
        if (fold_lanes<FW, 8>(part, ld, n_chunks, i4, i4 < n, red4, s4)) {
            float4 *o = reinterpret_cast<float4 *>(out + i4);
            if (acc) s4 = fold_add(s4, *o);
            *o = s4;
        }
        return;
    }
    const int64_t i = (int64_t)wg * 64 + el;
    float s;
    if (fold_lanes<FW, 8>(part, ld, n_chunks, i, i < n, red, s)) {
        const int r = (int)(i / cols), c = (int)(i - (int64_t)r * cols);
        float *o = out + (int64_t)r * out_ld + c;
        *o = acc ? *o + s : s;
    }
}

// ---- deferred finalizes: the closed forms (finalize.h) that nothing inside the backward waits for, in ONE launch behind the folds ---------
// Flat grid as above: workgroup b belongs to the record whose [wg0, wg0 + nwg) range holds it; 1024 threads, four output rows / channels each.
constexpr int FIN_MAX = 4;
struct FinBatch { papc_fold_fin f[FIN_MAX]; int wg0[FIN_MAX + 1], count; };
__global__ __launch_bounds__(1024) void fold_fin_kernel(FinBatch b)
{
    __shared__ double lds[DWMAX_FIN_LDS > XYZ_BWD_FIN_LDS ? DWMAX_FIN_LDS : XYZ_BWD_FIN_LDS];
    int r = 0;
    while (r + 1 < b.count && (int)blockIdx.x >= b.wg0[r + 1]) ++r;
    const int wg = (int)blockIdx.x - b.wg0[r];
    const papc_fold_fin &f = b.f[r];
    if (f.kind == PAPC_FIN_DW_MAX)
        dw_max_finalize_body(lds, wg, 1024, static_cast<const double *>(f.src), f.w, f.e, f.scale, f.c1, f.inv_m, f.C, f.dw, f.accumulate);
    else
        xyz_l1_bwd_finalize_body(lds, wg, static_cast<const float *>(f.src), f.parts, f.M, f.C, f.gram, f.w, f.ldw, f.xcol0, f.bias, f.mean, f.invstd,
                                 f.scale, f.dgamma, f.dbeta, f.dw, f.accumulate);
}

}  // namespace papc


using namespace papc;

static int launch_fins(const papc_fold_fin *fins, int count, hipStream_t st)
{
    // the records of one launch run concurrently and end in a read-modify-write of dw (dgamma, dbeta): a record that writes where an earlier one of
    // the launch does (a module applied twice in one backward pass) starts the next launch, so such records apply in list order
    for (int r0 = 0; r0 < count;) {
        FinBatch b;
        memset(&b, 0, sizeof(b));
        int n = 0, wgs = 0;
        for (; n < FIN_MAX && r0 + n < count; ++n) {
            const papc_fold_fin &f = fins[r0 + n];
            bool shared = false;
            for (int k = 0; k < n && !shared; ++k) shared = b.f[k].dw == f.dw || (f.dgamma && b.f[k].dgamma == f.dgamma) || (f.dbeta && b.f[k].dbeta == f.dbeta);
            if (shared) break;
            b.f[n] = f;
            b.wg0[n] = wgs;
            wgs += (int)cdiv(f.C, 4);
        }
        b.wg0[n] = wgs;
        b.count = n;
        ProfScope prof(PAPC_K_BWD_DW, st);
        hipLaunchKernelGGL(fold_fin_kernel, dim3((unsigned)wgs), dim3(1024), 0, st, b);
        const int rc = check_launch("papc_fold_jobs_f32 (finalizes)");
        if (rc != PAPC_OK) return rc;
        r0 += n;
    }
    return PAPC_OK;
}

// Two fold jobs whose output RANGES intersect can still write disjoint elements: column blocks of one row-major matrix (the same row stride:
// the xyz and the feature columns of the gather-add first layer's dW).  True only where that is certain.
static bool disjoint_column_blocks(const papc_fold_job &a, const papc_fold_job &b)
{
    if (a.rows < 2 || b.rows < 2 || a.out_ld != b.out_ld) return false;
    const bool a_first = (uintptr_t)a.out <= (uintptr_t)b.out;
    const papc_fold_job &p = a_first ? a : b, &q = a_first ? b : a;
    const uintptr_t bytes = (uintptr_t)q.out - (uintptr_t)p.out;
    if (bytes % sizeof(float)) return false;
    const int64_t c0 = (int64_t)(bytes / sizeof(float)) % p.out_ld;        // q's first column in p's row grid
    return c0 >= p.cols && c0 + q.cols <= p.out_ld;                        // (q's rows do not wrap; p holds columns [0, p.cols))
}

extern "C" {

int papc_reduce_partials2_f32(const float *partial, int n_chunks, int64_t ld, int64_t n1, float *out1, int64_t n2,
                              float *out2, int accumulate, papc_stream_t stream)
{
    PAPC_REQUIRE(partial && out1 && (n2 == 0 || out2), PAPC_E_INVALID, "papc_reduce_partials2_f32: null pointer");
    PAPC_REQUIRE(n_chunks >= 1 && n1 >= 1 && n2 >= 0 && ld >= n1 + n2, PAPC_E_INVALID, "papc_reduce_partials2_f32: bad sizes");
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    const int64_t n = n1 + n2;
    const bool wide = n_chunks <= 64 && n >= 16384 && n1 % 4 == 0 && n2 % 4 == 0 && ld % 4 == 0 && aligned16(partial) && aligned16(out1) &&
                      (n2 == 0 || aligned16(out2));
    if (wide)
        hipLaunchKernelGGL(reduce_partials_wide_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, partial, n_chunks, n, ld, out1, n1, out2, accumulate);
    else
        hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)cdiv(n, 64)), dim3(1024), 0, st, partial, n_chunks, n, ld, out1, n1, out2, accumulate);
    return check_launch("papc_reduce_partials2_f32");
}

int papc_reduce_partials_batch_f32(const papc_reduce_job *jobs, int count, papc_stream_t stream)
{
    PAPC_REQUIRE(jobs, PAPC_E_INVALID, "papc_reduce_partials_batch_f32: null jobs");
    PAPC_REQUIRE(count >= 1 && count <= 8, PAPC_E_INVALID, "papc_reduce_partials_batch_f32: count=%d not in [1, 8]", count);
    ReduceBatch b;
    memset(&b, 0, sizeof(b));
    int64_t nmax = 0;
    for (int i = 0; i < count; ++i) {
        const papc_reduce_job &j = jobs[i];
        PAPC_REQUIRE(j.partial && j.out1 && (j.n2 == 0 || j.out2), PAPC_E_INVALID, "papc_reduce_partials_batch_f32: null pointer in job %d", i);
        PAPC_REQUIRE(j.n_chunks >= 1 && j.n1 >= 1 && j.n2 >= 0 && j.ld >= j.n1 + j.n2, PAPC_E_INVALID, "papc_reduce_partials_batch_f32: bad sizes in job %d", i);
        b.part[i] = j.partial; b.out1[i] = j.out1; b.out2[i] = j.out2; b.ld[i] = j.ld; b.n1[i] = j.n1; b.n[i] = j.n1 + j.n2;
        b.n_chunks[i] = j.n_chunks; b.accumulate[i] = j.accumulate;
        nmax = std::max(nmax, j.n1 + j.n2);
    }
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(reduce_partials_batch_kernel, dim3((unsigned)cdiv(nmax, 64), (unsigned)count), dim3(1024), 0, st, b);
    return check_launch("papc_reduce_partials_batch_f32");
}

int papc_fold_jobs_f32(const papc_fold_job *list, int list_count, papc_stream_t stream)
{
    PAPC_REQUIRE(list, PAPC_E_INVALID, "papc_fold_jobs_f32: null jobs");
    PAPC_REQUIRE(list_count >= 1, PAPC_E_INVALID, "papc_fold_jobs_f32: count=%d", list_count);
    hipStream_t st = as_stream(stream);
    // the finalize records (a header slot + the record's bytes in the slots behind it) leave the list: they run behind every fold
    std::vector<papc_fold_job> folds;
    std::vector<papc_fold_fin> fins;
    for (int i = 0; i < list_count; ++i) {
        if (list[i].rows != PAPC_FOLD_FIN) { folds.push_back(list[i]); continue; }
        PAPC_REQUIRE(list[i].n_chunks == PAPC_FOLD_FIN_SLOTS && i + PAPC_FOLD_FIN_SLOTS < list_count, PAPC_E_INVALID, "papc_fold_jobs_f32: truncated finalize record at job %d", i);
        papc_fold_fin f;
        memcpy(&f, &list[i + 1], sizeof(f));
        PAPC_REQUIRE((f.kind == PAPC_FIN_DW_MAX || f.kind == PAPC_FIN_XYZ_BWD) && f.kind == list[i].cols && f.C >= 1 && f.src && f.dw, PAPC_E_INVALID,
                     "papc_fold_jobs_f32: bad finalize record at job %d", i);
        fins.push_back(f);
        i += PAPC_FOLD_FIN_SLOTS;
    }
    const papc_fold_job *jobs = folds.data();
    const int count = (int)folds.size();
    const int FW = knob(KNOB_FOLD_WAVES) == 16 ? 16 : 8;
    // The jobs of ONE launch run concurrently (a flat grid), and a job ends in a read-modify-write of its output: a launch holds only jobs
    // whose output ranges [out, out + (rows - 1) * out_ld + cols) are pairwise disjoint.  A job that overlaps one of the current launch
    // starts the next launch, so overlapping jobs apply in list order (a module applied twice in one backward pass queues two accumulate
    // jobs on the same .grad); a list without overlaps -- every step without sharing -- still folds in ceil(count / PAPC_FOLD_MAX) launches.
    for (int j0 = 0; j0 < count;) {
        FoldBatch b;
        memset(&b, 0, sizeof(b));
        int64_t wgs = 0;
        uintptr_t lo[PAPC_FOLD_MAX], hi[PAPC_FOLD_MAX];
        int nj = 0;
        for (; nj < PAPC_FOLD_MAX && j0 + nj < count; ++nj) {
            const int i = nj;
            papc_fold_job j = jobs[j0 + i];
            const bool f64 = j.rows == PAPC_FOLD_F64Q;       // one row of cols doubles
            if (f64) j.rows = 1;
            PAPC_REQUIRE(j.partial && j.out, PAPC_E_INVALID, "papc_fold_jobs_f32: null pointer in job %d", j0 + i);
            PAPC_REQUIRE(j.n_chunks >= 1 && j.rows >= 1 && j.cols >= 1 && j.ld >= (int64_t)j.rows * j.cols && j.out_ld >= j.cols, PAPC_E_INVALID,
                         "papc_fold_jobs_f32: bad sizes in job %d", j0 + i);
            PAPC_REQUIRE(!f64 || (!j.accumulate && ((uintptr_t)j.out & 7) == 0), PAPC_E_INVALID, "papc_fold_jobs_f32: bad float64 job %d", j0 + i);
            lo[i] = (uintptr_t)j.out;
            hi[i] = lo[i] + (f64 ? sizeof(double) : sizeof(float)) * (uintptr_t)((int64_t)(j.rows - 1) * j.out_ld + j.cols);
            bool overlaps = false;
            for (int k = 0; k < i && !overlaps; ++k)
                overlaps = lo[i] < hi[k] && lo[k] < hi[i] && !disjoint_column_blocks(jobs[j0 + k], j);
            if (overlaps) break;                // (i >= 1 here: the launch below is never empty)
            const int64_t n = (int64_t)j.rows * j.cols;
            const bool wide = !f64 && j.n_chunks <= 16 && n >= 16384 && n % 4 == 0 && j.ld % 4 == 0 && (j.rows == 1 || j.out_ld == j.cols) && aligned16(j.partial) && aligned16(j.out);
            b.part[i] = j.partial; b.out[i] = j.out; b.ld[i] = j.ld; b.out_ld[i] = j.out_ld; b.n_chunks[i] = j.n_chunks; b.rows[i] = j.rows; b.cols[i] = j.cols;
            if (j.accumulate) b.acc_mask |= 1u << i;
            const bool vec = !f64 && !wide && n >= 1024 && n % 4 == 0 && j.ld % 4 == 0 && (j.rows == 1 || j.out_ld == j.cols) && aligned16(j.partial) && aligned16(j.out);
            if (wide) b.wide_mask |= 1u << i;
            if (vec) b.vec_mask |= 1u << i;
            if (f64) b.f64_mask |= 1u << i;
            b.wg0[i] = (int)wgs;
            wgs += f64 ? cdiv(n, 16 * FW) : wide ? cdiv(n, 4 * 64 * FW) : (vec ? cdiv(n, 256) : cdiv(n, 64));
            PAPC_REQUIRE(wgs < (1ll << 30), PAPC_E_UNSUPPORTED, "papc_fold_jobs_f32: too many elements");
        }
        b.wg0[nj] = (int)wgs;
        b.count = nj;
        ProfScope prof(PAPC_K_BWD_DW, st);
        if (FW == 8) hipLaunchKernelGGL(fold_jobs_kernel<8>, dim3((unsigned)wgs), dim3(512), 0, st, b);
        else hipLaunchKernelGGL(fold_jobs_kernel<16>, dim3((unsigned)wgs), dim3(1024), 0, st, b);
        const int rc = check_launch("papc_fold_jobs_f32");
        if (rc != PAPC_OK) return rc;
        j0 += nj;
    }
    return fins.empty() ? PAPC_OK : launch_fins(fins.data(), (int)fins.size(), st);
}

int papc_reduce_partials_f32(const float *partial, int n_chunks, int64_t n, float *out, int accumulate, papc_stream_t stream)
{
    PAPC_REQUIRE(partial && out, PAPC_E_INVALID, "papc_reduce_partials_f32: null pointer");
    PAPC_REQUIRE(n_chunks >= 1 && n >= 1, PAPC_E_INVALID, "papc_reduce_partials_f32: bad sizes");
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)cdiv(n, 64)), dim3(1024), 0, st, partial, n_chunks, n, n, out, n, (float *)nullptr, accumulate);
    return check_launch("papc_reduce_partials_f32");
}

int papc_reduce_partials_strided_f32(const float *partial, int n_chunks, int64_t ld, int rows, int cols, float *out, int64_t out_ld,
                                     int accumulate, papc_stream_t stream)
{
    PAPC_REQUIRE(partial && out, PAPC_E_INVALID, "papc_reduce_partials_strided_f32: null pointer");
    PAPC_REQUIRE(n_chunks >= 1 && rows >= 1 && cols >= 1 && ld >= (int64_t)rows * cols && out_ld >= cols, PAPC_E_INVALID,
                 "papc_reduce_partials_strided_f32: bad sizes");
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(reduce_partials_strided_kernel, dim3((unsigned)cdiv((int64_t)rows * cols, 16)), dim3(1024), 0, st, partial, n_chunks, ld,
                       rows, cols, out, out_ld, accumulate);
    return check_launch("papc_reduce_partials_strided_f32");
}

}  // extern "C"
