// nms_iou.h -- the IoU device code of the NMS family, once: the order-preserving score key, the axis-aligned "+1" IoU and the rotated-box
// clipping routines.  Included by nms.hip (papc_nms_f32, papc_rotate_nms_f32, the IoU entry points) and detpost.hip (papc_det_post_f32).
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

}  // namespace papc
