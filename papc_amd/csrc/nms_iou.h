// nms_iou.h -- the device code of the NMS family, once: the order-preserving score key, the axis-aligned "+1" IoU, the rotated-box clipping
// routines, the stand-up box of a quadrilateral with its eps = 0 IoU (standup_of, standup_iou), and the two halves of bitmask NMS -- the
// 64x64 suppression-word tile (nms_mask_tile) and the sequential sweep over the words (nms_sweep).  Included by nms.hip (papc_nms_f32,
// papc_rotate_nms_f32: the tile on one wave, the sweep to the end; the IoU entry points), detpost.hip (papc_det_post_f32: the tile on
// DP_MASK_WAVES waves, the sweep stopped at post_max) and dettarget.hip (standup_iou is the assigner's similarity).
#pragma once
#include "common.h"

namespace papc {

__device__ __forceinline__ uint32_t ordered_f32(float f)   // order-preserving float -> uint32; -0.0 and +0.0 share one key (they
{                                                          // compare equal, so a stable argsort leaves them in index order)
    const uint32_t u = f == 0.f ? 0u : __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float iou_dev(const float *a, const float *b)   // nms_gpu.py:22-34
{
    const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
    const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
    const float width = fmaxf(right - left + 1.f, 0.f), height = fmaxf(bottom - top + 1.f, 0.f);
    const float interS = width * height;
    const float Sa = (a[2] - a[0] + 1.f) * (a[3] - a[1] + 1.f);
    const float Sb = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
    return interS / (Sa + Sb - interS);
}

// ---------------------------------------------------------------------------------------------------------------------
// rotated boxes (x, y, x_d, y_d, angle): IoU of two rectangles.  What the reference computes (nms_gpu.py:179-414, numba.cuda) is the
// area of a convex quadrilateral intersection; it gets there by collecting corner-in-box hits and edge-edge crossings, sorting them
// by angle around their centroid and summing a triangle fan.  This file does not follow that route.  Here box A is CLIPPED against
// the four half-planes of box B (Sutherland-Hodgman): the polygon stays an ordered vertex list throughout (at most 4 + 4 vertices),
// so there is no candidate list, no angular sort and no scratch array, and touching / coincident edges are ordinary cases of the
// signed-distance test instead of ties between strict comparisons (the source's IoU of two identical boxes at a general angle is
// rounding noise; here it is 1).  Corners are formed in fp32 exactly as the source forms them (:366-389: they define the rectangles);
// signed distances, crossing points and the shoelace sum are fp64, as are the area accumulator and the quotient in the source
// (`area_val = 0.0`, `/ 2.0` are Python floats under numba).  -ffp-contract=off.
// ---------------------------------------------------------------------------------------------------------------------
struct Quad { float x[4], y[4]; };

__device__ __forceinline__ Quad corners_of(const float *b)   // (x, y, x_d, y_d, angle) -> corners, the source's order and arithmetic (:366-389)
{
    const float c = cosf(b[4]), s = sinf(b[4]);
    const float hx = b[2] / 2.f, hy = b[3] / 2.f;
    Quad q;
    q.x[0] = c * -hx + s * -hy + b[0]; q.y[0] = -s * -hx + c * -hy + b[1];
    q.x[1] = c * -hx + s * hy + b[0];  q.y[1] = -s * -hx + c * hy + b[1];
    q.x[2] = c * hx + s * hy + b[0];   q.y[2] = -s * hx + c * hy + b[1];
    q.x[3] = c * hx + s * -hy + b[0];  q.y[3] = -s * hx + c * -hy + b[1];
    return q;
}

// twice the signed area of a quadrilateral (shoelace); its sign is the winding of the corner order
__device__ __forceinline__ double quad_area2(const Quad &q)
{
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3;
        a += (double)q.x[i] * (double)q.y[j] - (double)q.x[j] * (double)q.y[i];
    }
    return a;
}

// Area of (convex quadrilateral A) n (convex quadrilateral B).  The vertex list lives in eight named slots per coordinate; every index
// below is a compile-time constant after unrolling (a slot is picked with selects), so the lists stay in registers.
__device__ double quad_intersection_area(const Quad &A, const Quad &B)
{
    const double b2 = quad_area2(B);
    if (b2 == 0.0) return 0.0;                                 // B is a point or an axis-parallel segment: no interior (every distance below would be 0 = "inside")
    const double wind = b2 < 0.0 ? -1.0 : 1.0;                 // inside = left of every edge for counter-clockwise B, right for clockwise
    double px[8], py[8];
    int n = 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) { px[i] = i < 4 ? (double)A.x[i] : 0.0; py[i] = i < 4 ? (double)A.y[i] : 0.0; }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double cx = (double)B.x[e], cy = (double)B.y[e];
        const double ex = (double)B.x[(e + 1) & 3] - cx, ey = (double)B.y[(e + 1) & 3] - cy;
        // signed distance (times |edge|) of every live vertex to the edge's line, positive inside
        double sd[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) sd[i] = wind * (ex * (py[i] - cy) - ey * (px[i] - cx));
        double qx[8], qy[8];
        int m = 0;
        // the vertex before slot 0 is the last live one
        double lx = px[0], ly = py[0], ls = sd[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) if (i == n - 1) { lx = px[i]; ly = py[i]; ls = sd[i]; }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < n) {
                const double vx = px[i], vy = py[i], vs = sd[i];
                const bool in_v = vs >= 0.0, in_l = ls >= 0.0;
                if (in_v != in_l) {                            // the boundary is crossed between the previous vertex and this one
                    const double t = ls / (ls - vs);
                    const double ix = lx + t * (vx - lx), iy = ly + t * (vy - ly);
#pragma unroll
                    for (int k = 0; k < 8; ++k) if (k == m) { qx[k] = ix; qy[k] = iy; }
                    ++m;
                }
                if (in_v) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) if (k == m) { qx[k] = vx; qy[k] = vy; }
                    ++m;
                }
                lx = vx; ly = vy; ls = vs;
            }
        }
        n = m < 8 ? m : 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) { px[i] = qx[i]; py[i] = qy[i]; }
        if (n == 0) return 0.0;
    }
    // shoelace over the live vertices, relative to vertex 0 (keeps the products small)
    double a2 = 0.0;
#pragma unroll
    for (int i = 1; i < 7; ++i)
        if (i + 1 < n) a2 += (px[i] - px[0]) * (py[i + 1] - py[0]) - (px[i + 1] - px[0]) * (py[i] - py[0]);
    return fabs(a2) * 0.5;
}

__device__ __forceinline__ double rotate_inter(const float *b1, const float *b2)   // inter(), :392-406
{
    return quad_intersection_area(corners_of(b1), corners_of(b2));
}

__device__ __forceinline__ double rotate_iou_eval(const float *b1, const float *b2, int criterion)   // :409-414, :562-574
{
    const float area1 = b1[2] * b1[3], area2 = b2[2] * b2[3];
    const double ai = rotate_inter(b1, b2);
    if (criterion == -1) return ai / ((double)(area1 + area2) - ai);
    if (criterion == 0) return ai / (double)area1;
    if (criterion == 1) return ai / (double)area2;
    return ai;
}

// corner_to_standup_nd (box_np_ops.py:236-241, box_paddle_ops.py:202-209): the axis-aligned bounding box (x0, y0, x1, y1) of four corners
__device__ __forceinline__ float4 standup_of(const Quad &q)
{
    float x0 = q.x[0], y0 = q.y[0], x1 = q.x[0], y1 = q.y[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) { x0 = fminf(x0, q.x[k]); y0 = fminf(y0, q.y[k]); x1 = fmaxf(x1, q.x[k]); y1 = fmaxf(y1, q.y[k]); }
    return make_float4(x0, y0, x1, y1);
}

// iou_jit (box_np_ops.py:654-682) with eps = 0 for one pair of (x0, y0, x1, y1) boxes, operation for operation as it runs on float32 inputs;
// qarea = (q.z - q.x) * (q.w - q.y), which a caller with many boxes against one q forms once
__device__ __forceinline__ float standup_iou(const float4 &a, const float4 &q, float qarea)
{
    const float iw = fminf(a.z, q.z) - fmaxf(a.x, q.x);
    if (!(iw > 0.f)) return 0.f;
    const float ih = fminf(a.w, q.w) - fmaxf(a.y, q.y);
    if (!(ih > 0.f)) return 0.f;
    const float ua = (a.z - a.x) * (a.w - a.y) + qarea - iw * ih;
    return iw * ih / ua;
}

// ---- bitmask NMS (nms_gpu.py:73-108 nms_kernel, :417-450 rotate_nms_kernel, :111-127 nms_postprocess) on boxes sorted by descending score ----

// One (row block, column block) tile of suppression words: bit j of row i's word is set when IoU(box_i, box_j) > thr and, on the diagonal
// tile, j comes after i.  The reference builds the word with a 64-iteration loop per thread (threadsPerBlock = 64 = one mask word); on a
// 64-lane wave the word IS one __ballot over the block's columns.  A workgroup of WAVES waves runs the tile: 64 row boxes staged in LDS,
// one column box per lane, 64 / WAVES consecutive rows per wave (the same ballots whatever WAVES is).  boxes: row_stride floats per box, the
// first five (x0, y0, x1, y1, -) or (x, y, x_d, y_d, angle); mask_row0: the word of (row 0, block 0).  Which tiles run is the caller's business.
template <bool ROTATE, int WAVES>
__device__ __forceinline__ void nms_mask_tile(const float *__restrict__ boxes, int row_stride, int N, float thr, int row_start, int col_start,
                                              unsigned long long *__restrict__ mask_row0, int col_blocks)
{
    constexpr int ROWS = 64 / WAVES;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    __shared__ float rows[64 * 5];
    const int row_size = min(N - row_start * 64, 64), col_size = min(N - col_start * 64, 64);
    if (wave == 0 && lane < row_size) {
#pragma unroll
        for (int c = 0; c < 5; ++c) rows[lane * 5 + c] = boxes[((int64_t)row_start * 64 + lane) * row_stride + c];
    }
    float cb[5] = {0.f, 0.f, 1.f, 1.f, 0.f};
    if (lane < col_size) {
#pragma unroll
        for (int c = 0; c < 5; ++c) cb[c] = boxes[((int64_t)col_start * 64 + lane) * row_stride + c];
    }
    __syncthreads();
    unsigned long long mine = 0;
    const int row0 = wave * ROWS, row1 = min(row0 + ROWS, row_size);
    for (int i = row0; i < row1; ++i) {
        const int start = (row_start == col_start) ? i + 1 : 0;                                   // :96-98
        bool hit = false;
        if (lane >= start && lane < col_size) {
            if (ROTATE) hit = rotate_iou_eval(&rows[i * 5], cb, -1) > (double)thr;                // devRotateIoU(cur, block_box) (:443-446)
            else hit = iou_dev(&rows[i * 5], cb) > thr;                                           // :99-102
        }
        const unsigned long long t = __ballot(hit);
        if (lane == i) mine = t;
    }
    if (lane >= row0 && lane < row1) mask_row0[((int64_t)row_start * 64 + lane) * col_blocks + col_start] = mine;   // :105
}

// nms_postprocess (:111-127) on one wave (64 threads): keep box i unless an earlier kept box removed it, until `limit` are kept.  mask: the
// tiles' words, col_blocks per row -- only the words from a row's own block on are read, up to block ceil(N / 64) - 1.  remv: the caller's
// LDS, ceil(N / 64) words, zeroed here; lanes OR a kept row's words in parallel.  record(n, i), called by lane 0: box i is the n-th kept.
template <class Record>
__device__ __forceinline__ int nms_sweep(const unsigned long long *__restrict__ mask, int N, int col_blocks, int limit, unsigned long long *remv,
                                         Record record)
{
    const int lane = threadIdx.x, words = (N + 63) >> 6;
    for (int j = lane; j < words; j += 64) remv[j] = 0ull;
    __syncthreads();
    int n_keep = 0;
    for (int i = 0; i < N && n_keep < limit; ++i) {
        const int nblock = i >> 6, inblock = i & 63;
        const bool removed = (remv[nblock] >> inblock) & 1ull;      // uniform (same LDS word for every lane)
        if (!removed) {
            if (lane == 0) record(n_keep, i);
            ++n_keep;
            for (int j = nblock + lane; j < words; j += 64) remv[j] |= mask[(int64_t)i * col_blocks + j];
            __syncthreads();                                        // in a branch every lane takes or none does: `removed` is uniform
        }
    }
    return n_keep;
}

}  // namespace papc
