// nms.hip -- axis-aligned bitmask NMS for gfx950.
//
// Reference: /root/reference/PAPC/models/detect/pointpillars/libs/ops/non_max_suppression/nms_gpu.py:22-34 (iou_device),
// :73-108 (nms_kernel), :111-127 (nms_postprocess), :130-164 (nms_gpu); C++/CUDA twin libs/ops/cc/nms/nms_kernel.cu.cc:38-157.
//
//   order  = argsort(score) descending                       (radix sort of (ordered score, index) keys, rocPRIM)
//   mask   = per (row box i, 64-column block) one 64-bit word: bit j set when IoU(box_i, box_j) > thr and j comes after i
//            -- nms_mask_tile (nms_iou.h), one wave per tile, every tile of the grid
//   sweep  = the reference's sequential host loop (keep i unless an earlier kept box removed it), one wave on the device
//            -- nms_sweep (nms_iou.h), run to the last box
// The tile and the sweep are the ones papc_det_post_f32 (detpost.hip) runs.  The rotated variant (papc_rotate_nms_f32) and the IoU entry
// points (rotate_iou, rbbox_iou, riou: the stand-up pre-test is standup_of / standup_iou of nms_iou.h) live here too.
// IoU in fp32 with the source's "+1" box convention, -ffp-contract=off: the keep decisions are bit-identical to the oracle.
#include "carve.h"
#include "common.h"
#include "nms_iou.h"
#include <rocprim/rocprim.hpp>

namespace papc {

__global__ __launch_bounds__(256) void nms_key_kernel(const float *__restrict__ dets, int N, int W, uint64_t *__restrict__ keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) keys[i] = ((uint64_t)ordered_f32(dets[(int64_t)i * W + W - 1]) << 32) | (uint32_t)i;   // score = last column
}

__global__ __launch_bounds__(256) void nms_gather_kernel(const float *__restrict__ dets, const uint64_t *__restrict__ keys, int N, int W,
                                                         float *__restrict__ sorted, int32_t *__restrict__ order)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int src = (int)(uint32_t)keys[i];
    order[i] = src;
    for (int c = 0; c < W; ++c) sorted[(int64_t)i * W + c] = dets[(int64_t)src * W + c];
}

// one wave per (row block, column block), every tile of the cb x cb grid: nms_mask_tile (nms_iou.h) on the sorted rows, [N,5] =
// (x1, y1, x2, y2, score) for nms_kernel (:73-108), [N,6] = (x, y, x_d, y_d, angle, score) for rotate_nms_kernel (:417-450)
template <bool ROTATE>
__global__ __launch_bounds__(64) void nms_mask_kernel(const float *__restrict__ boxes, int N, float thr, int col_blocks,
                                                      unsigned long long *__restrict__ mask)
{
    nms_mask_tile<ROTATE, 1>(boxes, ROTATE ? 6 : 5, N, thr, blockIdx.y, blockIdx.x, mask, col_blocks);
}

// nms_postprocess (:111-127) on one wave: nms_sweep (nms_iou.h) over all N boxes, remv words in dynamic LDS
__global__ __launch_bounds__(64) void nms_sweep_kernel(const unsigned long long *__restrict__ mask, const int32_t *__restrict__ order, int N,
                                                       int col_blocks, int32_t *__restrict__ keep, int32_t *__restrict__ num_out)
{
    extern __shared__ unsigned long long remv[];
    const int n_keep = nms_sweep(mask, N, col_blocks, N, remv, [&](int n, int i) { keep[n] = order[i]; });   // list(order[keep])  (:164)
    if (threadIdx.x == 0) num_out[0] = n_keep;
}

// rotate_iou_kernel(_eval) (:491-521, :577-615): iou[n, k] = devRotateIoUEval(query[k], boxes[n], criterion)
__global__ __launch_bounds__(256) void rotate_iou_kernel(const float *__restrict__ boxes, const float *__restrict__ query, int N, int K,
                                                         int criterion, float *__restrict__ iou)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)N * K) return;
    const int n = (int)(e / K), k = (int)(e - (int64_t)n * K);
    float q[5], b[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) { q[c] = query[(int64_t)k * 5 + c]; b[c] = boxes[(int64_t)n * 5 + c]; }
    iou[e] = (float)rotate_iou_eval(q, b, criterion);
}

// rbbox_iou (cc/box_ops.h:23-80, boost::geometry on the host in the reference): overlaps[n, k] = area(P_n n Q_k) / area(P_n u Q_k) for the
// pairs whose axis-aligned "standup" IoU exceeds standup_thresh, 0 elsewhere.  Convex quadrilaterals: the union's area is
// |P| + |Q| - |P n Q|.  CORNERS = false: the boxes arrive as (x, y, w, l, angle) and the corners (center_to_corner_box2d, box_np_ops.py:363-383:
// the same rotation as rbbox_to_corners), the standup boxes (:236-241) and their IoU (iou_jit with eps = 0, :654-682) are formed here --
// riou_cc (:16-27) in one launch.
template <bool CORNERS>
__global__ __launch_bounds__(256) void rbbox_iou_kernel(const float *__restrict__ boxes, const float *__restrict__ qboxes,
                                                        const float *__restrict__ standup_iou, float standup_thresh, int N, int K,
                                                        float *__restrict__ overlaps)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)N * K) return;
    const int n = (int)(e / K), k = (int)(e - (int64_t)n * K);
    Quad P, Q;
    if (CORNERS) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            P.x[i] = boxes[(int64_t)n * 8 + 2 * i]; P.y[i] = boxes[(int64_t)n * 8 + 2 * i + 1];
            Q.x[i] = qboxes[(int64_t)k * 8 + 2 * i]; Q.y[i] = qboxes[(int64_t)k * 8 + 2 * i + 1];
        }
    } else {
        float b[5], q[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) { b[c] = boxes[(int64_t)n * 5 + c]; q[c] = qboxes[(int64_t)k * 5 + c]; }
        P = corners_of(b);
        Q = corners_of(q);
    }
    float su;
    if (CORNERS && standup_iou) su = standup_iou[e];
    else {
        const float4 p = standup_of(P), q = standup_of(Q);
        su = papc::standup_iou(p, q, (q.z - q.x) * (q.w - q.y));      // (the parameter of that name is the caller's precomputed matrix)
    }
    float out = 0.f;
    if (su > standup_thresh) {
        const double ai = quad_intersection_area(P, Q);
        if (ai > 0.0) {
            const double un = fabs(quad_area2(P)) * 0.5 + fabs(quad_area2(Q)) * 0.5 - ai;
            if (un > 0.0) out = (float)(ai / un);
        }
    }
    overlaps[e] = out;
}

}  // namespace papc

using namespace papc;

extern "C" {

// workspace of both drivers: [keys | sorted keys | boxes N x 6 | order | suppression mask N x cb | rocPRIM's temporary storage]
struct NmsPtrs { uint64_t *keys, *sorted_keys; float *boxes; int32_t *order; unsigned long long *mask; void *tmp; size_t sort_bytes = 0; };
static size_t nms_layout(int N, void *base, hipStream_t st, NmsPtrs &p)
{
    WsCarver c = WsCarver::over(base);
    p.keys = c.take<uint64_t>((size_t)N); p.sorted_keys = c.take<uint64_t>((size_t)N);
    p.boxes = c.take<float>((size_t)N * 6); p.order = c.take<int32_t>((size_t)N);
    p.mask = c.take<unsigned long long>((size_t)N * cdiv(N, 64));
    (void)rocprim::radix_sort_keys_desc(nullptr, p.sort_bytes, p.keys, p.sorted_keys, (size_t)N, 0, 64, st);
    p.tmp = c.take<char>(p.sort_bytes);
    return c.bytes();
}

size_t papc_nms_workspace(int N)
{
    NmsPtrs p;
    return N < 1 ? 0 : nms_layout(N, nullptr, (hipStream_t)0, p);
}

static int nms_driver(const float *dets, int N, int W, float thr, int32_t *keep, int32_t *num_out, void *workspace, size_t workspace_bytes,
                      papc_stream_t stream, const char *who)
{
    PAPC_REQUIRE(dets && keep && num_out && workspace, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(N >= 1 && N <= 65536, PAPC_E_INVALID, "%s: N=%d not in [1, 65536]", who, N);
    hipStream_t st = as_stream(stream);
    NmsPtrs p;
    PAPC_REQUIRE(workspace_bytes >= nms_layout(N, workspace, st, p), PAPC_E_INVALID, "%s: workspace too small", who);
    ProfScope prof(PAPC_K_MISC, st);
    const int cb = cdiv(N, 64);
    const unsigned nb = (unsigned)cdiv(N, 256);
    hipLaunchKernelGGL(nms_key_kernel, dim3(nb), dim3(256), 0, st, dets, N, W, p.keys);
    // descending (score, index): scores.argsort()[::-1] with a stable sort (:145, :469)
    if (rocprim::radix_sort_keys_desc(p.tmp, p.sort_bytes, p.keys, p.sorted_keys, (size_t)N, 0, 64, st) != hipSuccess) return check_launch(who);
    hipLaunchKernelGGL(nms_gather_kernel, dim3(nb), dim3(256), 0, st, dets, p.sorted_keys, N, W, p.boxes, p.order);
    if (W == 5) hipLaunchKernelGGL(nms_mask_kernel<false>, dim3((unsigned)cb, (unsigned)cb), dim3(64), 0, st, p.boxes, N, thr, cb, p.mask);
    else hipLaunchKernelGGL(nms_mask_kernel<true>, dim3((unsigned)cb, (unsigned)cb), dim3(64), 0, st, p.boxes, N, thr, cb, p.mask);
    hipLaunchKernelGGL(nms_sweep_kernel, dim3(1), dim3(64), (size_t)cb * 8, st, p.mask, p.order, N, cb, keep, num_out);
    return check_launch(who);
}

int papc_nms_f32(const float *dets, int N, float nms_overlap_thresh, int32_t *keep, int32_t *num_out, void *workspace,
                 size_t workspace_bytes, papc_stream_t stream)
{
    return nms_driver(dets, N, 5, nms_overlap_thresh, keep, num_out, workspace, workspace_bytes, stream, "papc_nms_f32");
}

int papc_rotate_nms_f32(const float *dets, int N, float nms_overlap_thresh, int32_t *keep, int32_t *num_out, void *workspace,
                        size_t workspace_bytes, papc_stream_t stream)
{
    return nms_driver(dets, N, 6, nms_overlap_thresh, keep, num_out, workspace, workspace_bytes, stream, "papc_rotate_nms_f32");
}

int papc_rotate_iou_f32(const float *boxes, const float *query_boxes, int N, int K, int criterion, float *iou, papc_stream_t stream)
{
    PAPC_REQUIRE(boxes && query_boxes && iou, PAPC_E_INVALID, "papc_rotate_iou_f32: null pointer");
    PAPC_REQUIRE(N >= 1 && K >= 1 && criterion >= -1 && criterion <= 2, PAPC_E_INVALID, "papc_rotate_iou_f32: N=%d K=%d criterion=%d", N, K, criterion);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(rotate_iou_kernel, dim3((unsigned)cdiv((int64_t)N * K, 256)), dim3(256), 0, st, boxes, query_boxes, N, K, criterion, iou);
    return check_launch("papc_rotate_iou_f32");
}

int papc_rbbox_iou_f32(const float *box_corners, const float *qbox_corners, const float *standup_iou, float standup_thresh, int N, int K,
                       float *overlaps, papc_stream_t stream)
{
    PAPC_REQUIRE(box_corners && qbox_corners && overlaps, PAPC_E_INVALID, "papc_rbbox_iou_f32: null pointer");
    PAPC_REQUIRE(N >= 1 && K >= 1, PAPC_E_INVALID, "papc_rbbox_iou_f32: N=%d K=%d", N, K);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(rbbox_iou_kernel<true>, dim3((unsigned)cdiv((int64_t)N * K, 256)), dim3(256), 0, st, box_corners, qbox_corners, standup_iou,
                       standup_thresh, N, K, overlaps);
    return check_launch("papc_rbbox_iou_f32");
}

int papc_riou_f32(const float *rbboxes, const float *qrbboxes, float standup_thresh, int N, int K, float *overlaps, papc_stream_t stream)
{
    PAPC_REQUIRE(rbboxes && qrbboxes && overlaps, PAPC_E_INVALID, "papc_riou_f32: null pointer");
    PAPC_REQUIRE(N >= 1 && K >= 1, PAPC_E_INVALID, "papc_riou_f32: N=%d K=%d", N, K);
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(rbbox_iou_kernel<false>, dim3((unsigned)cdiv((int64_t)N * K, 256)), dim3(256), 0, st, rbboxes, qrbboxes, (const float *)nullptr,
                       standup_thresh, N, K, overlaps);
    return check_launch("papc_riou_f32");
}

}  // extern "C"
