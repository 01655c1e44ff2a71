// detpost.hip -- PointPillars predict(): decode, score, top-k and NMS for a whole batch on the device (gfx950).
//
// Reference: pointpillars/models/detectors/pointpillars.py:218-398 (predict, the non-multiclass path :319-360 and the direction fix :367-374) with
// libs/ops/box_paddle_ops.py:48-83 (second_box_decode), :151-185, :242-257, :286-305 (center_to_corner_box2d), :202-209 (corner_to_standup_nd),
// :394-442 (nms / rotate_nms: top-k, the NMS call, [:post_max_size]).
//
//   score   every anchor: class scores, top score and label, the threshold; a passing anchor writes a sort key, a failing one a key that sorts
//           behind every passing key of its frame; num_pass[b] by one integer atomic per wave.  No box is decoded here.
//   order   ONE device-wide descending radix sort (rocPRIM) of keys (B - 1 - b | score | a): frame b's keys land in [b A, (b + 1) A), inside
//           it by descending score, then descending anchor index -- the order of nms_key_kernel, which the top-k cut and the sweep share
//   decode  ranks < n_b = min(num_pass[b], K) only: second_box_decode in the source's fp32 operation order (box_decode, box_codec.h), the NMS
//           box (the rotated one, or its stand-up box: standup_of, nms_iou.h), score, label, direction label
//   mask    grid (cb, cb, B), cb = ceil(K / 64): nms_mask_tile (nms_iou.h), the tile papc_nms_f32 / papc_rotate_nms_f32 run, on eight
//           waves; blocks past n_b and blocks left of the diagonal (never read by the sweep) exit
//   sweep   one wave per frame: nms_sweep (nms_iou.h), the standalone drivers' sequential loop, stopped at P kept boxes, then the outputs,
//           padding included
// papc_box_decode_f32, the elementwise decode, is box_codec.h's driver.
// Nothing here waits on the host: n_b is read from device memory by every kernel that needs it.  -ffp-contract=off.
#include "box_codec.h"
#include "carve.h"
#include "common.h"
#include "nms_iou.h"
#include <rocprim/rocprim.hpp>

namespace papc {

struct DpArgs {
    papc_det_post_desc d;
    papc_det_post_io io;
    int abits, cb;                       // bits of an anchor index in a key; mask words per row
    uint64_t *keys, *sorted;             // [B A]
    float *nbox, *box7, *score;          // candidates: [B K 5] NMS boxes, [B K 7] decoded boxes, [B K]
    int32_t *label, *dirl, *aidx;        // [B K]
    unsigned long long *mask;            // [B K cb]
};

__device__ __forceinline__ float dp_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }   // F.sigmoid

// total_scores (:258-267) and its (max, argmax) (:322-326) for one anchor; strict > keeps the lowest class on exactly equal scores
__device__ __forceinline__ float dp_top_score(const float *__restrict__ cls, int num_cls, int mode, int &label)
{
    const int c0 = mode == 0 ? 0 : 1;
    float best, mx = 0.f, sum = 1.f;
    if (mode == 2) {
        mx = cls[0];
        for (int c = 1; c < num_cls; ++c) mx = fmaxf(mx, cls[c]);
        sum = 0.f;
        for (int c = 0; c < num_cls; ++c) sum += expf(cls[c] - mx);
    }
    best = mode == 2 ? expf(cls[c0] - mx) / sum : dp_sigmoid(cls[c0]);
    label = 0;
    for (int c = c0 + 1; c < num_cls; ++c) {
        const float s = mode == 2 ? expf(cls[c] - mx) / sum : dp_sigmoid(cls[c]);
        if (s > best) { best = s; label = c - c0; }
    }
    return best;
}

// key = (B - 1 - b) << (31 + abits) | field << abits | a: field 0 = failed, else 1 + the score's ordered bits without their sign bit (scores
// are sigmoids / softmax terms, never negative: 31 bits hold them)
__global__ __launch_bounds__(256) void dp_score_kernel(DpArgs a)
{
    const papc_det_post_desc &d = a.d;
    const int b = blockIdx.y, lane = lane_id();
    const uint64_t frame = (uint64_t)(d.B - 1 - b) << (31 + a.abits);
    for (int base = blockIdx.x * 256; base < d.A; base += gridDim.x * 256) {        // uniform per block: the ballot below sees whole waves
        const int i = base + threadIdx.x;
        bool pass = false;
        if (i < d.A) {
            const int64_t g = (int64_t)b * d.A + i;
            int label;
            const float s = dp_top_score(a.io.cls_preds + g * d.num_cls, d.num_cls, d.score_mode, label);
            pass = (!a.io.anchors_mask || a.io.anchors_mask[g] != 0) && (d.score_thresh <= 0.f || s >= d.score_thresh);   // :251-256, :328-331
            const uint64_t field = pass ? (uint64_t)(ordered_f32(s) & 0x7fffffffu) + 1u : 0u;
            a.keys[g] = frame | (field << a.abits) | (uint32_t)i;
        }
        const unsigned long long m = __ballot(pass);
        if (lane == 0 && m) atomicAdd(&a.io.num_pass[b], (int)__popcll(m));
    }
}

__device__ __forceinline__ int dp_nb(const DpArgs &a, int b) { return min(a.io.num_pass[b], a.d.pre_max); }   // nms(): min(len(scores), pre_max_size)

__global__ __launch_bounds__(256) void dp_gather_kernel(DpArgs a)
{
    const papc_det_post_desc &d = a.d;
    const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
    if (r >= dp_nb(a, b)) return;
    const int i = (int)(a.sorted[(int64_t)b * d.A + r] & ((1ull << a.abits) - 1ull));
    const int64_t g = (int64_t)b * d.A + i, c = (int64_t)b * d.pre_max + r;
    const int code = d.code_size;
    float t[8], an[7], o[7];
#pragma unroll
    for (int k = 0; k < 8; ++k) t[k] = k < code ? a.io.box_preds[g * code + k] : 0.f;
    const float *anchors = a.io.anchors + (int64_t)b * d.anchor_batch_stride + (int64_t)i * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) an[k] = anchors[k];
    box_decode(t, an, d.encode_angle_to_vector, d.smooth_dim, o);
#pragma unroll
    for (int k = 0; k < 7; ++k) a.box7[c * 7 + k] = o[k];
    float nb[5] = {o[0], o[1], o[3], o[4], o[6]};                        // box_preds[:, [0, 1, 3, 4, 6]]  (:338)
    if (!d.use_rotate_nms) {                                             // center_to_corner_box2d -> corner_to_standup_nd (:339-344); corners_of
        const float4 su = standup_of(corners_of(nb));                    // is that rotation, term for term (dims * -+0.5, x cos + y sin, + centre)
        nb[0] = su.x; nb[1] = su.y; nb[2] = su.z; nb[3] = su.w; nb[4] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) a.nbox[c * 5 + k] = nb[k];
    int label;
    a.score[c] = dp_top_score(a.io.cls_preds + g * d.num_cls, d.num_cls, d.score_mode, label);    // the bits the key was made of
    a.label[c] = label;
    a.dirl[c] = d.use_dir ? (a.io.dir_preds[g * 2 + 1] > a.io.dir_preds[g * 2] ? 1 : 0) : 0;     // argmax(dir_preds, -1), first entry on a tie (:257)
    a.aidx[c] = i;
}

// one workgroup per (row block, column block, frame): nms_mask_tile (nms_iou.h) on frame b's n_b candidates.  The standalone drivers walk a
// block's 64 rows on one wave; K = 1000 leaves 136 blocks per frame on the diagonal and right of it, and a rotated IoU is a long fp64 chain, so
// here DP_MASK_WAVES waves share the rows, 64 / DP_MASK_WAVES consecutive ones each (the same ballots).
constexpr int DP_MASK_WAVES = 8;
template <bool ROTATE>
__global__ __launch_bounds__(64 * DP_MASK_WAVES) void dp_mask_kernel(DpArgs a)
{
    const int row_start = blockIdx.y, col_start = blockIdx.x, b = blockIdx.z;
    if (col_start < row_start) return;                                  // left of the diagonal: the sweep reads words from its own block on
    const int N = dp_nb(a, b);                                          // (those blocks leave before this load)
    if (col_start * 64 >= N) return;
    nms_mask_tile<ROTATE, DP_MASK_WAVES>(a.nbox + (int64_t)b * a.d.pre_max * 5, 5, N, a.d.iou_thresh, row_start, col_start,
                                         a.mask + (int64_t)b * a.d.pre_max * a.cb, a.cb);
}

// nms_postprocess on one wave per frame (nms_sweep, nms_iou.h), stopped at P kept boxes ([:post_max_size], :410), then every output row of the frame
__global__ __launch_bounds__(64) void dp_sweep_emit_kernel(DpArgs a)
{
    const papc_det_post_desc &d = a.d;
    __shared__ unsigned long long remv[64];
    __shared__ int kept[4096];
    const int b = blockIdx.x, lane = threadIdx.x, K = d.pre_max, P = d.post_max;
    const int N = min(dp_nb(a, b), 64 * 64);                        // pre_max <= 4096: said again, so that the sweep's strided loops are one pass
    const int n_keep = nms_sweep(a.mask + (int64_t)b * K * a.cb, N, a.cb, P, remv, [&](int n, int i) { kept[n] = i; });
    __syncthreads();
    if (lane == 0) a.io.num_det[b] = n_keep;
    const float pi = 3.14159265358979323846f;                       // np.pi cast to the boxes' dtype (:372)
    for (int p = lane; p < P; p += 64) {
        const int64_t o = (int64_t)b * P + p;
        if (p < n_keep) {
            const int64_t c = (int64_t)b * K + kept[p];
#pragma unroll
            for (int k = 0; k < 6; ++k) a.io.boxes[o * 7 + k] = a.box7[c * 7 + k];
            float r = a.box7[c * 7 + 6];
            const int dl = a.dirl[c];
            if (d.use_dir && ((r > 0.f) != (dl != 0))) r += pi;     // :369-374
            a.io.boxes[o * 7 + 6] = r;
            a.io.scores[o] = a.score[c];
            a.io.labels[o] = a.label[c];
            a.io.dir_labels[o] = dl;
            a.io.anchor_idx[o] = a.aidx[c];
        } else {
#pragma unroll
            for (int k = 0; k < 7; ++k) a.io.boxes[o * 7 + k] = 0.f;
            a.io.scores[o] = 0.f;
            a.io.labels[o] = 0;
            a.io.dir_labels[o] = 0;
            a.io.anchor_idx[o] = -1;
        }
    }
}

}  // namespace papc

using namespace papc;

static int dp_check_desc(const char *who, const papc_det_post_desc *d)
{
    PAPC_REQUIRE(d, PAPC_E_INVALID, "%s: null pointer", who);
    if (int rc = require_frames_anchors(who, d->B, d->A)) return rc;
    if (int rc = require_code_size(who, d->code_size, d->encode_angle_to_vector)) return rc;
    PAPC_REQUIRE(d->score_mode >= 0 && d->score_mode <= 2, PAPC_E_INVALID, "%s: score_mode=%d not in {0, 1, 2}", who, d->score_mode);
    PAPC_REQUIRE(d->num_cls >= (d->score_mode == 0 ? 1 : 2) && d->num_cls <= 16, PAPC_E_INVALID,
                 "%s: num_cls=%d not in [%d, 16] for score_mode %d", who, d->num_cls, d->score_mode == 0 ? 1 : 2, d->score_mode);
    PAPC_REQUIRE(d->pre_max >= 1 && d->pre_max <= 4096, PAPC_E_INVALID, "%s: pre_max=%d not in [1, 4096]", who, d->pre_max);
    PAPC_REQUIRE(d->post_max >= 1 && d->post_max <= d->pre_max, PAPC_E_INVALID, "%s: post_max=%d not in [1, pre_max=%d]", who, d->post_max, d->pre_max);
    PAPC_REQUIRE(d->anchor_batch_stride >= 0, PAPC_E_INVALID, "%s: anchor_batch_stride=%lld < 0", who, (long long)d->anchor_batch_stride);
    return 0;
}

static int dp_bits(int64_t n)      // bits that hold every value in [0, n)
{
    int bits = 0;
    while (((int64_t)1 << bits) < n) ++bits;
    return bits;
}

// workspace: [keys | sorted keys | NMS boxes | decoded boxes | score | label | dir label | anchor | suppression words | rocPRIM's temporary storage]
static size_t dp_layout(const papc_det_post_desc *d, void *base, hipStream_t st, DpArgs &a, void *&tmp, size_t &sort_bytes, int &end_bit)
{
    const size_t BA = (size_t)d->B * d->A, BK = (size_t)d->B * d->pre_max;
    a.d = *d;
    a.abits = dp_bits(d->A);
    a.cb = (int)cdiv(d->pre_max, 64);
    end_bit = 31 + a.abits + dp_bits(d->B);                              // <= 63: B * A < 2^31
    WsCarver c = WsCarver::over(base);
    a.keys = c.take<uint64_t>(BA); a.sorted = c.take<uint64_t>(BA);
    a.nbox = c.take<float>(BK * 5); a.box7 = c.take<float>(BK * 7); a.score = c.take<float>(BK);
    a.label = c.take<int32_t>(BK); a.dirl = c.take<int32_t>(BK); a.aidx = c.take<int32_t>(BK);
    a.mask = c.take<unsigned long long>(BK * a.cb);
    sort_bytes = 0;
    (void)rocprim::radix_sort_keys_desc(nullptr, sort_bytes, a.keys, a.sorted, BA, 0, end_bit, st);
    tmp = c.take<char>(sort_bytes);
    return c.bytes();
}

extern "C" {

size_t papc_det_post_workspace(const papc_det_post_desc *desc)
{
    if (dp_check_desc("papc_det_post_workspace", desc) != 0) return (size_t)-1;
    DpArgs a;
    void *tmp;
    size_t sort_bytes;
    int end_bit;
    return dp_layout(desc, nullptr, (hipStream_t)0, a, tmp, sort_bytes, end_bit);
}

int papc_det_post_f32(const papc_det_post_desc *desc, const papc_det_post_io *io, void *workspace, size_t workspace_bytes, papc_stream_t stream)
{
    const char *who = "papc_det_post_f32";
    int rc = dp_check_desc(who, desc);
    if (rc != 0) return rc;
    PAPC_REQUIRE(io && workspace, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(io->box_preds && io->cls_preds && io->anchors && (io->dir_preds || !desc->use_dir), PAPC_E_INVALID, "%s: null input pointer", who);
    PAPC_REQUIRE(io->boxes && io->scores && io->labels && io->dir_labels && io->anchor_idx && io->num_det && io->num_pass, PAPC_E_INVALID,
                 "%s: null output pointer", who);
    hipStream_t st = as_stream(stream);
    DpArgs a;
    void *tmp;
    size_t sort_bytes;
    int end_bit;
    PAPC_REQUIRE(workspace_bytes >= dp_layout(desc, workspace, st, a, tmp, sort_bytes, end_bit), PAPC_E_INVALID, "%s: workspace too small", who);
    a.io = *io;
    ProfScope prof(PAPC_K_MISC, st);
    const papc_det_post_desc &d = *desc;
    const unsigned B = (unsigned)d.B;
    if (hipMemsetAsync(io->num_pass, 0, (size_t)d.B * sizeof(int32_t), st) != hipSuccess) return check_launch(who);
    const unsigned score_blocks = (unsigned)std::min<int64_t>(cdiv(d.A, 256), std::max<int64_t>(1, 2048 / d.B));
    hipLaunchKernelGGL(dp_score_kernel, dim3(score_blocks, B), dim3(256), 0, st, a);
    // descending (frame, score, anchor): per frame scores.argsort()[::-1] with a stable sort, the order papc_nms_f32 sweeps in
    if (rocprim::radix_sort_keys_desc(tmp, sort_bytes, a.keys, a.sorted, (size_t)d.B * d.A, 0, end_bit, st) != hipSuccess) return check_launch(who);
    hipLaunchKernelGGL(dp_gather_kernel, dim3((unsigned)cdiv(d.pre_max, 256), B), dim3(256), 0, st, a);
    if (d.use_rotate_nms) hipLaunchKernelGGL(dp_mask_kernel<true>, dim3((unsigned)a.cb, (unsigned)a.cb, B), dim3(64 * DP_MASK_WAVES), 0, st, a);
    else hipLaunchKernelGGL(dp_mask_kernel<false>, dim3((unsigned)a.cb, (unsigned)a.cb, B), dim3(64 * DP_MASK_WAVES), 0, st, a);
    hipLaunchKernelGGL(dp_sweep_emit_kernel, dim3(B), dim3(64), 0, st, a);
    return check_launch(who);
}

int papc_box_decode_f32(const float *enc, const float *anchors, int64_t n, int code_size, int encode_angle_to_vector, int smooth_dim, float *out,
                        papc_stream_t stream)
{
    return box_codec_launch<false>("papc_box_decode_f32", enc, anchors, n, code_size, encode_angle_to_vector, smooth_dim, out, stream);
}

}  // extern "C"
