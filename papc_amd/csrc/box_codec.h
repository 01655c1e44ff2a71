// box_codec.h -- the SECOND box code, both directions side by side: second_box_encode (box_np_ops.py:30-66) and its inverse second_box_decode
// (box_paddle_ops.py:48-83), each in its source's fp32 operation order (-ffp-contract=off), the one elementwise kernel and host driver behind
// papc_box_encode_f32 (dettarget.hip) and papc_box_decode_f32 (detpost.hip), and the two argument checks the detection entry points share
// (require_code_size; require_frames_anchors: a (frame, anchor) pair is indexed in 32 bits, a frame by a grid dimension).
// dt_decide_kernel (dettarget.hip) encodes with box_encode, dp_gather_kernel (detpost.hip) decodes with box_decode.
#pragma once
#include "common.h"

namespace papc {

// second_box_encode (box_np_ops.py:30-66), the source's operation order in fp32
__device__ __forceinline__ void box_encode(const float *__restrict__ bx, const float *__restrict__ an, int angle_vec, int smooth, float *o)
{
    const float xa = an[0], ya = an[1], wa = an[3], la = an[4], ha = an[5], ra = an[6];
    const float xg = bx[0], yg = bx[1], wg = bx[3], lg = bx[4], hg = bx[5], rg = bx[6];
    const float zg = bx[2] + hg / 2.f, za = an[2] + ha / 2.f;            // :41-42
    const float diagonal = sqrtf(la * la + wa * wa);                      // :43
    o[0] = (xg - xa) / diagonal;                                          // :44-45
    o[1] = (yg - ya) / diagonal;
    o[2] = (zg - za) / ha;                                                // :47
    if (smooth) { o[4] = lg / la - 1.f; o[3] = wg / wa - 1.f; o[5] = hg / ha - 1.f; }               // :48-51
    else { o[4] = logf(lg / la); o[3] = logf(wg / wa); o[5] = logf(hg / ha); }                      // :52-55
    if (angle_vec) { o[6] = cosf(rg) - cosf(ra); o[7] = sinf(rg) - sinf(ra); }                      // :56-63
    else o[6] = rg - ra;                                                  // :65
}

// second_box_decode (box_paddle_ops.py:48-83), the source's operation order in fp32
__device__ __forceinline__ void box_decode(const float *__restrict__ t, const float *__restrict__ an, int angle_vec, int smooth, float *o)
{
    const float xa = an[0], ya = an[1], wa = an[3], la = an[4], ha = an[5], ra = an[6];
    const float za = an[2] + ha / 2.f;                                   // :61
    const float diagonal = sqrtf(la * la + wa * wa);                     // :62
    const float xg = t[0] * diagonal + xa, yg = t[1] * diagonal + ya;    // :63-64
    float zg = t[2] * ha + za;                                           // :65
    float lg, wg, hg, rg;
    if (smooth) { lg = (t[4] + 1.f) * la; wg = (t[3] + 1.f) * wa; hg = (t[5] + 1.f) * ha; }        // :66-69
    else { lg = expf(t[4]) * la; wg = expf(t[3]) * wa; hg = expf(t[5]) * ha; }                     // :70-73
    if (angle_vec) rg = atan2f(t[7] + sinf(ra), t[6] + cosf(ra));        // :74-79
    else rg = t[6] + ra;                                                 // :81
    zg = zg - hg / 2.f;                                                  // :82
    o[0] = xg; o[1] = yg; o[2] = zg; o[3] = wg; o[4] = lg; o[5] = hg; o[6] = rg;
}

// one box per thread: [n, 7] boxes -> [n, code] encodings (ENCODE) or back; anchors [n, 7]
template <bool ENCODE>
__global__ __launch_bounds__(256) void box_codec_kernel(const float *__restrict__ in, const float *__restrict__ anchors, int64_t n, int code,
                                                        int angle_vec, int smooth, float *__restrict__ out)
{
    constexpr int IN = ENCODE ? 7 : 8, OUT = ENCODE ? 8 : 7;             // registers; `code` of the 8 are in memory
    const int in_w = ENCODE ? 7 : code, out_w = ENCODE ? code : 7;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float v[IN], an[7], o[OUT];
#pragma unroll
        for (int c = 0; c < IN; ++c) v[c] = c < in_w ? in[i * in_w + c] : 0.f;
#pragma unroll
        for (int c = 0; c < 7; ++c) an[c] = anchors[i * 7 + c];
        if (ENCODE) box_encode(v, an, angle_vec, smooth, o);
        else box_decode(v, an, angle_vec, smooth, o);
#pragma unroll
        for (int c = 0; c < OUT; ++c)
            if (c < out_w) out[i * out_w + c] = o[c];
    }
}

static inline int require_code_size(const char *who, int code_size, int encode_angle_to_vector)
{
    PAPC_REQUIRE(code_size == (encode_angle_to_vector ? 8 : 7), PAPC_E_INVALID, "%s: code_size=%d with encode_angle_to_vector=%d (8 iff set, else 7)",
                 who, code_size, encode_angle_to_vector);
    return 0;
}

static inline int require_frames_anchors(const char *who, int B, int A)
{
    PAPC_REQUIRE(B >= 1 && B <= 65535 && A >= 1 && (int64_t)B * A < ((int64_t)1 << 31), PAPC_E_INVALID,
                 "%s: B=%d A=%d (need 1 <= B <= 65535, A >= 1 and B * A < 2^31)", who, B, A);
    return 0;
}

template <bool ENCODE>      // papc_box_encode_f32 / papc_box_decode_f32
static int box_codec_launch(const char *who, const float *in, const float *anchors, int64_t n, int code_size, int angle_vec, int smooth, float *out,
                            papc_stream_t stream)
{
    PAPC_REQUIRE(in && anchors && out, PAPC_E_INVALID, "%s: null pointer", who);
    PAPC_REQUIRE(n >= 1, PAPC_E_INVALID, "%s: n=%lld < 1", who, (long long)n);
    if (int rc = require_code_size(who, code_size, angle_vec)) return rc;
    hipStream_t st = as_stream(stream);
    ProfScope prof(PAPC_K_MISC, st);
    hipLaunchKernelGGL(box_codec_kernel<ENCODE>, dim3((unsigned)std::min<int64_t>(cdiv(n, 256), 2048)), dim3(256), 0, st, in, anchors, n, code_size,
                       angle_vec != 0, smooth != 0, out);
    return check_launch(who);
}

}  // namespace papc
