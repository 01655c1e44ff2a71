// dettarget.hip -- PointPillars training targets on the device: the occupied-area anchor mask and TargetAssigner.assign (gfx950).
//
// Reference: data/preprocess.py:251-302 with libs/ops/box_np_ops.py:772-805 (sparse_sum_for_anchors_mask, the two cumsums, fused_get_anchors_area),
// libs/ops/target_ops.py:31-214 (create_target_np, the positive_fraction=None path), core/similarity_calculator.py:73-93 with box_np_ops.py:244-256,
// :654-682 (rbbox2d_to_near_bbox, iou_jit with eps = 0) and box_np_ops.py:30-66 (second_box_encode).
//
//   mask    count   one integer vector atomic per coors row into the int32 map [B, ny, nx] (rows with a batch index outside [0, B) skipped)
//           rows    inclusive prefix sum along x, one wave per map row
//           cols    inclusive prefix sum along y, a workgroup per 64 columns, a run of rows per wave
//           area    per (frame, anchor): S[y2,x2] - S[y2,x1] - S[y1,x2] + S[y1,x1] on the anchor's cached cell box; mask = area > threshold
//   assign  gmax    per-gt maximum overlap over the inside anchors: LDS max per workgroup, one global atomic max per (workgroup, gt) with a
//                   non-zero maximum.  IoU >= 0, so the float's bits order as unsigned integers; a max does not depend on the order.
//           decide  the G overlaps again per anchor: max / argmax (lowest gt on ties), the force match, the label, second_box_encode
// Integers make the mask exact.  The overlap is canonical fp32, operation for operation as iou_jit runs on float32 inputs: no fused multiply-add
// (-ffp-contract=off), IEEE division.  Nothing here waits on the host.
// The overlap is standup_iou (nms_iou.h, shared with the rbbox_iou / riou pre-test), second_box_encode is box_encode (box_codec.h, beside its
// inverse); papc_box_encode_f32, the elementwise encode, is box_codec.h's driver.
#include "box_codec.h"
#include "carve.h"
#include "common.h"
#include "nms_iou.h"

namespace papc {

struct AmArgs {
    papc_anchors_mask_desc d;
    papc_anchors_mask_io io;
    int32_t *map;                        // [B, ny, nx]: counts, then their inclusive 2-D prefix sums, in place
};

__global__ __launch_bounds__(256) void am_count_kernel(AmArgs a)
{
    const papc_anchors_mask_desc &d = a.d;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < d.P; i += (int64_t)gridDim.x * 256) {
        const int4 c = reinterpret_cast<const int4 *>(a.io.coors)[i];          // (batch, z, y, x)
        if (c.x < 0 || c.x >= d.B || c.z < 0 || c.z >= d.ny || c.w < 0 || c.w >= d.nx) continue;
        atomicAdd(&a.map[((int64_t)c.x * d.ny + c.z) * d.nx + c.w], 1);       // duplicates count twice, as ret[y, x] += 1 does
    }
}

// cumsum(1): one wave per row, 64 columns at a time with the carry of the columns before
__global__ __launch_bounds__(256) void am_row_scan_kernel(AmArgs a)
{
    const papc_anchors_mask_desc &d = a.d;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)d.B * d.ny) return;
    const int lane = lane_id();
    int32_t *p = a.map + row * d.nx;
    int carry = 0;
    for (int x0 = 0; x0 < d.nx; x0 += 64) {
        const int x = x0 + lane;
        int v = x < d.nx ? p[x] : 0;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int u = __shfl_up(v, s);
            if (lane >= s) v += u;
        }
        v += carry;
        if (x < d.nx) p[x] = v;
        carry = __shfl(v, 63);
    }
}

// cumsum(0): a workgroup per (frame, 64 columns); its AM_SEG waves each take a run of rows -- the run's column sums first (loads only, so they
// pipeline), the sums of the runs above through LDS, then the prefix written eight rows per round trip
constexpr int AM_SEG = 16;
__global__ __launch_bounds__(64 * AM_SEG) void am_col_scan_kernel(AmArgs a)
{
    const papc_anchors_mask_desc &d = a.d;
    __shared__ int seg_sum[AM_SEG][64];
    const int lane = lane_id(), seg = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane, b = blockIdx.y;
    const int rows = (d.ny + AM_SEG - 1) / AM_SEG, y0 = min(seg * rows, d.ny), y1 = min(y0 + rows, d.ny);
    const bool live = x < d.nx;
    int32_t *p = a.map + (int64_t)b * d.ny * d.nx + (live ? x : 0);
    int sum = 0;
    if (live)
        for (int y = y0; y < y1; ++y) sum += p[(int64_t)y * d.nx];
    seg_sum[seg][lane] = sum;
    __syncthreads();
    int acc = 0;
    for (int s = 0; s < seg; ++s) acc += seg_sum[s][lane];
    if (!live) return;
    for (int y = y0; y < y1; y += 8) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = y + k < y1 ? p[(int64_t)(y + k) * d.nx] : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            acc += v[k];
            if (y + k < y1) p[(int64_t)(y + k) * d.nx] = acc;
        }
    }
}

__global__ __launch_bounds__(256) void am_area_kernel(AmArgs a)
{
    const papc_anchors_mask_desc &d = a.d;
    const int b = blockIdx.y;
    const int32_t *S = a.map + (int64_t)b * d.ny * d.nx;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < d.A; i += gridDim.x * 256) {
        int4 c = reinterpret_cast<const int4 *>(a.io.cells)[i];                // (x1, y1, x2, y2); the caller keeps them inside the grid, and no
        c.x = min(max(c.x, 0), d.nx - 1); c.z = min(max(c.z, 0), d.nx - 1);   // read leaves the map whatever it passes
        c.y = min(max(c.y, 0), d.ny - 1); c.w = min(max(c.w, 0), d.ny - 1);
        const int ID = S[(int64_t)c.w * d.nx + c.z], IA = S[(int64_t)c.y * d.nx + c.x];
        const int IB = S[(int64_t)c.w * d.nx + c.x], IC = S[(int64_t)c.y * d.nx + c.z];
        const int area = ID - IB - IC + IA;                                   // box_np_ops.py:800-804: the min cell's row and column are left out
        a.io.mask[(int64_t)b * d.A + i] = (float)area > d.area_thresh ? 1 : 0;
    }
}

struct DtArgs {
    papc_det_assign_desc d;
    papc_det_assign_io io;
    unsigned *gmax;                      // [B, Gmax] bits of the per-gt maximum overlap over the inside anchors
};

constexpr int DT_GMAX = 256;

// rbbox2d_to_near_bbox (:244-256) of one box (x, y, w, l, r) read from a 7-float row: limit_period, the swap, centre -+ dims / 2
__device__ __forceinline__ void dt_near_bbox(const float *__restrict__ b7, float *o)
{
    const float pi = 3.14159265358979323846f, quarter = 0.78539816339744830962f;
    const float r = b7[6];
    const float lim = r - floorf(r / pi + 0.5f) * pi;                     // limit_period(rots, 0.5, np.pi)
    const bool swap = fabsf(lim) > quarter;
    const float dx = swap ? b7[4] : b7[3], dy = swap ? b7[3] : b7[4];
    o[0] = b7[0] - dx / 2.f; o[1] = b7[1] - dy / 2.f; o[2] = b7[0] + dx / 2.f; o[3] = b7[1] + dy / 2.f;
}

// the frame's gt near-bboxes and areas into LDS; returns G = num_gt[b] held to [0, Gmax]
__device__ __forceinline__ int dt_load_gts(const DtArgs &a, int b, float4 *qbv, float *qarea)
{
    const int G = min(max(a.io.num_gt[b], 0), a.d.Gmax);
    for (int g = threadIdx.x; g < G; g += blockDim.x) {
        float o[4];
        dt_near_bbox(a.io.gt_boxes + ((int64_t)b * a.d.Gmax + g) * 7, o);
        qbv[g] = make_float4(o[0], o[1], o[2], o[3]);
        qarea[g] = (o[2] - o[0]) * (o[3] - o[1]);
    }
    return G;
}

__global__ __launch_bounds__(256) void dt_gmax_kernel(DtArgs a)
{
    const papc_det_assign_desc &d = a.d;
    __shared__ float4 qbv[DT_GMAX];
    __shared__ float qarea[DT_GMAX];
    __shared__ unsigned lmax[DT_GMAX];
    const int b = blockIdx.y;
    const int G = dt_load_gts(a, b, qbv, qarea);
    if (G == 0) return;                                                   // uniform per block
    for (int g = threadIdx.x; g < G; g += 256) lmax[g] = 0u;
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < d.A; i += gridDim.x * 256) {
        if (a.io.anchors_mask && a.io.anchors_mask[(int64_t)b * d.A + i] == 0) continue;
        const float4 an = reinterpret_cast<const float4 *>(a.io.anchors_bv)[i];
        for (int g = 0; g < G; ++g) {
            const unsigned bits = __float_as_uint(standup_iou(an, qbv[g], qarea[g]));
            if (bits > lmax[g]) atomicMax(&lmax[g], bits);
        }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += 256)
        if (lmax[g] != 0u) atomicMax(&a.gmax[(int64_t)b * d.Gmax + g], lmax[g]);
}

template <bool ANGLE_VEC>      // a template parameter: the sinf / cosf of the angle-vector code stay out of the 7-float kernel
__global__ __launch_bounds__(256) void dt_decide_kernel(DtArgs a)
{
    const papc_det_assign_desc &d = a.d;
    __shared__ float4 qbv[DT_GMAX];
    __shared__ float qarea[DT_GMAX], gm[DT_GMAX];
    __shared__ int32_t qcls[DT_GMAX];
    const int b = blockIdx.y, lane = lane_id(), code = d.code_size;
    const int G = dt_load_gts(a, b, qbv, qarea);
    for (int g = threadIdx.x; g < G; g += 256) {
        const unsigned bits = a.gmax[(int64_t)b * d.Gmax + g];
        gm[g] = bits == 0u ? -1.f : __uint_as_float(bits);                // target_ops.py:109-110: a gt no inside anchor overlaps forces nothing
        qcls[g] = a.io.gt_classes[(int64_t)b * d.Gmax + g];
    }
    __syncthreads();
    for (int base = blockIdx.x * 256; base < d.A; base += gridDim.x * 256) {         // uniform per block: the ballot below sees whole waves
        const int i = base + threadIdx.x;
        bool pos = false;
        if (i < d.A) {
            const int64_t o = (int64_t)b * d.A + i;
            const bool inside = !a.io.anchors_mask || a.io.anchors_mask[o] != 0;
            int label = inside ? 0 : -1, aarg = 0;                        // :155-156: no gt, every inside anchor is a negative
            float amax = 0.f;
            if (inside && G > 0) {
                const float4 an = reinterpret_cast<const float4 *>(a.io.anchors_bv)[i];
                bool force = false;
                for (int g = 0; g < G; ++g) {
                    const float ov = standup_iou(an, qbv[g], qarea[g]);
                    if (g == 0 || ov > amax) { amax = ov; aarg = g; }     // np.argmax: the first of equal maxima
                    force |= ov == gm[g];
                }
                // :117-125, :158-160 in the order the source writes the labels: matched, then background, then the forced ones again
                if (force) label = qcls[aarg];
                else if (amax < a.io.unmatched[i]) label = 0;
                else if (amax >= a.io.matched[i]) label = qcls[aarg];
                else label = -1;
            }
            pos = label > 0;
            float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (pos) box_encode(a.io.gt_boxes + ((int64_t)b * d.Gmax + aarg) * 7, a.io.anchors + (int64_t)i * 7, ANGLE_VEC, d.smooth_dim, t);
            a.io.labels[o] = label;
#pragma unroll
            for (int c = 0; c < 8; ++c)                                   // constant indices: t stays in registers
                if (c < code) a.io.reg_targets[o * code + c] = t[c];
            a.io.reg_weights[o] = pos ? 1.f : 0.f;
            if (a.io.gt_ids) a.io.gt_ids[o] = pos ? aarg : -1;
            if (a.io.max_overlap) a.io.max_overlap[o] = amax;
        }
        if (a.io.num_pos) {
            const unsigned long long m = __ballot(pos);
            if (lane == 0 && m) atomicAdd(&a.io.num_pos[b], (int)__popcll(m));
        }
    }
}

}  // namespace papc

using namespace papc;

static int am_check_desc(const char *who, const papc_anchors_mask_desc *d)
{
    PAPC_REQUIRE(d, PAPC_E_INVALID, "%s: null pointer", who);
    if (int rc = require_frames_anchors(who, d->B, d->A)) return rc;
    PAPC_REQUIRE(d->ny >= 1 && d->nx >= 1 && (int64_t)d->B * d->ny * d->nx < ((int64_t)1 << 31), PAPC_E_INVALID,
                 "%s: ny=%d nx=%d (need ny >= 1, nx >= 1 and B * ny * nx < 2^31)", who, d->ny, d->nx);
    PAPC_REQUIRE(d->P >= 0, PAPC_E_INVALID, "%s: P=%lld < 0", who, (long long)d->P);
    return 0;
}

// workspace: [count map / prefix sums]
static size_t am_layout(const papc_anchors_mask_desc *d, void *base, AmArgs &a)
{
    a.d = *d;
    WsCarver c = WsCarver::over(base);
    a.map = c.take<int32_t>((size_t)d->B * d->ny * d->nx);
    return c.bytes();
}

static int dt_check_desc(const char *who, const papc_det_assign_desc *d)
{
    PAPC_REQUIRE(d, PAPC_E_INVALID, "%s: null pointer", who);
    if (int rc = require_frames_anchors(who, d->B, d->A)) return rc;
    PAPC_REQUIRE(d->Gmax >= 0 && d->Gmax <= DT_GMAX, PAPC_E_INVALID, "%s: Gmax=%d not in [0, %d]", who, d->Gmax, DT_GMAX);
    if (int rc = require_code_size(who, d->code_size, d->encode_angle_to_vector)) return rc;
    return 0;
}

// workspace: [per-gt maximum overlap bits]
static size_t dt_layout(const papc_det_assign_desc *d, void *base, DtArgs &a)
{
    a.d = *d;
    WsCarver c = WsCarver::over(base);
    a.gmax = c.take<unsigned>((size_t)d->B * std::max(d->Gmax, 1));
    return c.bytes();
}

extern "C" {

size_t papc_anchors_mask_workspace(const papc_anchors_mask_desc *desc)
{
    if (am_check_desc("papc_anchors_mask_workspace", desc) != 0) return (size_t)-1;
    AmArgs a;
    return am_layout(desc, nullptr, a);
}

int papc_anchors_mask_u8(const papc_anchors_mask_desc *desc, const papc_anchors_mask_io *io, void *workspace, size_t workspace_bytes,
                         papc_stream_t stream)
{
    const char *who = "papc_anchors_mask_u8";
    int rc = am_check_desc(who, desc);
    if (rc != 0) return rc;
    PAPC_REQUIRE(io && workspace, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE((io->coors || desc->P == 0) && io->cells, PAPC_E_INVALID, "%s: null input pointer", who);
    PAPC_REQUIRE(io->mask, PAPC_E_INVALID, "%s: null output pointer", who);
    PAPC_REQUIRE(aligned16(io->coors) && aligned16(io->cells), PAPC_E_INVALID, "%s: coors and cells must be 16-byte aligned", who);
    AmArgs a;
    PAPC_REQUIRE(workspace_bytes >= am_layout(desc, workspace, a), PAPC_E_INVALID, "%s: workspace too small", who);
    a.io = *io;
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    const papc_anchors_mask_desc &d = *desc;
    const unsigned B = (unsigned)d.B;
    if (hipMemsetAsync(a.map, 0, (size_t)d.B * d.ny * d.nx * sizeof(int32_t), st) != hipSuccess) return check_launch(who);
    if (d.P > 0) hipLaunchKernelGGL(am_count_kernel, dim3((unsigned)std::min<int64_t>(cdiv(d.P, 256), 2048)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(am_row_scan_kernel, dim3((unsigned)cdiv((int64_t)d.B * d.ny, 4)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(am_col_scan_kernel, dim3((unsigned)cdiv(d.nx, 64), B), dim3(64 * AM_SEG), 0, st, a);
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(d.A, 256), std::max<int64_t>(1, 2048 / d.B));
    hipLaunchKernelGGL(am_area_kernel, dim3(blocks, B), dim3(256), 0, st, a);
    return check_launch(who);
}

size_t papc_det_assign_workspace(const papc_det_assign_desc *desc)
{
    if (dt_check_desc("papc_det_assign_workspace", desc) != 0) return (size_t)-1;
    DtArgs a;
    return dt_layout(desc, nullptr, a);
}

int papc_det_assign_f32(const papc_det_assign_desc *desc, const papc_det_assign_io *io, void *workspace, size_t workspace_bytes,
                        papc_stream_t stream)
{
    const char *who = "papc_det_assign_f32";
    int rc = dt_check_desc(who, desc);
    if (rc != 0) return rc;
    PAPC_REQUIRE(io && workspace, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(io->anchors && io->anchors_bv && io->matched && io->unmatched && io->num_gt && ((io->gt_boxes && io->gt_classes) || desc->Gmax == 0),
                 PAPC_E_INVALID, "%s: null input pointer", who);
    PAPC_REQUIRE(io->labels && io->reg_targets && io->reg_weights, PAPC_E_INVALID, "%s: null output pointer", who);
    PAPC_REQUIRE(aligned16(io->anchors_bv), PAPC_E_INVALID, "%s: anchors_bv must be 16-byte aligned", who);
    DtArgs a;
    PAPC_REQUIRE(workspace_bytes >= dt_layout(desc, workspace, a), PAPC_E_INVALID, "%s: workspace too small", who);
    a.io = *io;
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    const papc_det_assign_desc &d = *desc;
    const unsigned B = (unsigned)d.B;
    if (hipMemsetAsync(a.gmax, 0, (size_t)d.B * std::max(d.Gmax, 1) * sizeof(unsigned), st) != hipSuccess) return check_launch(who);
    if (io->num_pos && hipMemsetAsync(io->num_pos, 0, (size_t)d.B * sizeof(int32_t), st) != hipSuccess) return check_launch(who);
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(d.A, 256), std::max<int64_t>(1, 2048 / d.B));
    if (d.Gmax > 0) hipLaunchKernelGGL(dt_gmax_kernel, dim3(blocks, B), dim3(256), 0, st, a);
    if (d.encode_angle_to_vector) hipLaunchKernelGGL(dt_decide_kernel<true>, dim3(blocks, B), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(dt_decide_kernel<false>, dim3(blocks, B), dim3(256), 0, st, a);
    return check_launch(who);
}

int papc_box_encode_f32(const float *boxes, const float *anchors, int64_t n, int code_size, int encode_angle_to_vector, int smooth_dim, float *out,
                        papc_stream_t stream)
{
    return box_codec_launch<true>("papc_box_encode_f32", boxes, anchors, n, code_size, encode_angle_to_vector, smooth_dim, out, stream);
}

}  // extern "C"
