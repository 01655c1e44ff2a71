// detloss.hip -- the PointPillars detection loss (pointpillars/models/detectors/pointpillars.py:150-213 with prepare_loss_weights :468-506,
// create_loss :508-549, add_sin_difference :551-557, _get_pos_neg_loss :559-573, get_direction_target :575-585, on core/losses.py's smooth
// L1 :151-183, sigmoid focal :253-292 / weighted sigmoid :205-231 and weighted softmax :370-391) as three launches:
//
//   dl_count_kernel   per 1024 labels: the exact (positives, negatives) counts as int32 partials, and the `cared` bytes
//   dl_main_kernel    per 256 anchors of one sample: folds its sample's count partials (integers: order-free), stages the 7-wide rows through
//                     LDS (flat coalesced loads and stores; a row is read at stride 7 dwords, conflict-free), computes the three terms and
//                     the three gradients for upstream gradient 1, and writes one partial row of DL_SLOTS sums
//   dl_fold_kernel    one workgroup: the lane fold of fold.h over the partial rows, eight rows to a chunk of 64 elements, then the eight
//                     sub-totals of a slot in order, then the scalars
//
// No float atomics and no data-dependent order: the same inputs give the same bits.  The counts never leave the device.
#include "carve.h"
#include "common.h"
#include "fold.h"

namespace papc {

constexpr int DL_T = 256;        // anchors (= threads) per workgroup of the main pass
constexpr int DL_CNT = 1024;     // labels per workgroup of the count pass
constexpr int DL_SLOTS = 8;      // floats of a partial row: sum loc, sum cls, sum dir, sum cls_pos, sum cls_neg, 0, 0, 0
constexpr int DL_CMAX = 8;
constexpr int DL_ROWS_PER_CHUNK = 64 / DL_SLOTS;

struct DlArgs {
    papc_det_loss_desc d;
    papc_det_loss_io io;
    int nblk, ncb, nrows, nchunks;     // main workgroups per sample, count workgroups per sample, B * nblk, cdiv(nrows, 8)
    int32_t *counts, *cnt_part;
    float *part;
};

template <typename LT>
__global__ __launch_bounds__(256) void dl_count_kernel(const LT *__restrict__ labels, int A, int ncb, int32_t *__restrict__ cnt_part,
                                                        uint8_t *__restrict__ cared)
{
    __shared__ int s_cnt[4][2];
    const int b = blockIdx.y, cb = blockIdx.x, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)b * A;
    int np = 0, nn = 0;
#pragma unroll
    for (int j = 0; j < DL_CNT / 256; ++j) {
        const int a = cb * DL_CNT + j * 256 + (int)threadIdx.x;
        const bool in = a < A;
        const LT L = in ? labels[row + a] : (LT)-1;
        np += __popcll(__ballot(L > 0));
        nn += __popcll(__ballot(L == 0));
        if (cared && in) cared[row + a] = L >= 0 ? 1 : 0;
    }
    if (lane_id() == 0) { s_cnt[wave][0] = np; s_cnt[wave][1] = nn; }
    __syncthreads();
    if (threadIdx.x < 2)
        cnt_part[((int64_t)b * ncb + cb) * 2 + threadIdx.x] = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
}

// softplus(z) = max(z, 0) + log1p(exp(-|z|)) and both sigmoids of z from one exponential: sg = sigmoid(z), sgn = sigmoid(-z)
__device__ __forceinline__ void dl_sigmoids(float z, float &sg, float &sgn, float &l1p)
{
    const float e = expf(-fabsf(z));
    const float r = 1.f / (1.f + e);
    sg = z >= 0.f ? r : e * r;
    sgn = z >= 0.f ? e * r : r;
    l1p = log1pf(e);
}

template <typename LT>
__global__ __launch_bounds__(DL_T) void dl_main_kernel(const DlArgs a)
{
    __shared__ float s_box[DL_T * 7], s_tgt[DL_T * 7];
    extern __shared__ float s_dyn[];                   // 2 * DL_T * (C | 1) floats: the logits (then their gradients), the per-class losses
    __shared__ float s_red[DL_T / 64][DL_SLOTS];
    __shared__ int s_np, s_nn;
    const papc_det_loss_desc &d = a.d;
    const int t = threadIdx.x, w = blockIdx.x;
    if (w >= a.nrows) {       // the rows that pad the last chunk of 64 elements: the fold adds their 0.f
        if (t < DL_SLOTS) a.part[(int64_t)w * DL_SLOTS + t] = 0.f;
        return;
    }
    const int b = w / a.nblk, blk = w - b * a.nblk;
    const int A = d.A, C = d.C, Cp = C | 1;            // odd LDS row stride: a row per lane without bank conflicts
    const int a0 = blk * DL_T, nv = min(DL_T, A - a0);
    const int64_t base = (int64_t)b * A + a0;
    float *s_cls = s_dyn, *s_cl2 = s_dyn + DL_T * Cp;

    if (t == 0) { s_np = 0; s_nn = 0; }
    // flat, coalesced loads of the 7-wide and C-wide rows
    {
        const float *gb = a.io.box_preds + base * 7, *gt = a.io.reg_targets + base * 7;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int i = t + DL_T * j;
            if (i < nv * 7) { s_box[i] = gb[i]; s_tgt[i] = gt[i]; }
        }
        const float *gc = a.io.cls_preds + base * C;
        for (int i = t; i < nv * C; i += DL_T) s_cls[(i / C) * Cp + i % C] = gc[i];
    }
    // this lane's own operands, in flight across the barriers below
    int64_t L = -1;
    float2 lg = make_float2(0.f, 0.f);
    float anc6 = 0.f;
    if (t < nv) {
        L = (int64_t)reinterpret_cast<const LT *>(a.io.labels)[base + t];
        if (d.has_dir) {
            lg = reinterpret_cast<const float2 *>(a.io.dir_preds)[base + t];
            anc6 = a.io.anchors[(base + t) * 7 + 6];
        }
    }
    int pnp = 0, pnn = 0;
    for (int i = t; i < a.ncb; i += DL_T) {
        pnp += a.cnt_part[((int64_t)b * a.ncb + i) * 2];
        pnn += a.cnt_part[((int64_t)b * a.ncb + i) * 2 + 1];
    }
    __syncthreads();
    if (pnp) atomicAdd(&s_np, pnp);      // integer adds in LDS: exact in any order
    if (pnn) atomicAdd(&s_nn, pnn);
    __syncthreads();
    const int np = s_np, nn = s_nn;
    if (blk == 0 && t == 0) { a.counts[2 * b] = np; a.counts[2 * b + 1] = nn; }

    float sum_loc = 0.f, sum_cls = 0.f, sum_dir = 0.f, sum_pos = 0.f, sum_neg = 0.f;
    if (t < nv) {
        const bool pos = L > 0, neg = L == 0;
        const float fB = (float)d.B;
        // prepare_loss_weights (:475-501); every normaliser is clipped at 1
        const float posn = fmaxf((float)np, 1.f);
        float cn = posn;
        if (d.norm_type == PAPC_DET_NORM_BY_NUM_EXAMPLES) cn = fmaxf((float)(np + nn), 1.f);
        else if (d.norm_type == PAPC_DET_NORM_BY_NUM_POS_NEG) cn = fmaxf(pos ? (float)np : neg ? (float)nn : 0.f, 1.f);
        const float cw = (d.neg_cls_weight + d.pos_cls_weight * (pos ? 1.f : 0.f)) / cn;       // don't-care anchors included (:480)
        const float rw = (pos ? 1.f : 0.f) / posn;

        // sigmoid focal loss on one-hot targets without the background column (losses.py:277-292); gamma = 0 without alpha is the
        // weighted sigmoid loss (:229-231).  z = the logit with the target's sign flipped: ce = softplus(z), 1 - p_t = sigmoid(z).
        const float gcls = d.cls_weight / fB;
        for (int c = 0; c < C; ++c) {
            const float x = s_cls[t * Cp + c];
            const bool tg = L == c + 1;
            float q, pt, l1p;
            dl_sigmoids(tg ? -x : x, q, pt, l1p);
            const float ce = fmaxf(x, 0.f) - (tg ? x : 0.f) + l1p;
            float mod = 1.f;
            if (d.gamma == 2.f) mod = q * q;
            else if (d.gamma != 0.f) mod = powf(q, d.gamma);
            const float af = d.has_alpha ? (tg ? d.alpha : 1.f - d.alpha) : 1.f;
            const float l = mod * af * ce * cw;
            const float dz = af * cw * mod * (d.gamma * pt * ce + q);       // d q^g / dz = g q^g (1 - q): no division by q
            s_cls[t * Cp + c] = gcls * (tg ? -dz : dz);
            s_cl2[t * Cp + c] = l;
            sum_cls += l;
            if (C == 1) { sum_pos += pos ? l : 0.f; sum_neg += neg ? l : 0.f; }        // _get_pos_neg_loss (:564-571)
            else if (c == 0) sum_neg += l;
            else sum_pos += l;
        }

        const float tgt6 = s_tgt[t * 7 + 6];
        // smooth L1, codewise (losses.py:166-177) behind add_sin_difference (:551-557)
        const float s2 = d.sigma * d.sigma, knee = 1.f / s2, half_knee = 0.5f / s2;
        const float gloc = d.loc_weight / fB;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const float p = s_box[t * 7 + k], g = s_tgt[t * 7 + k];
            float diff = p - g, jac = 1.f;
            if (k == 6 && d.sin_diff) {
                float sp, cp, st, ct;
                sincosf(p, &sp, &cp);
                sincosf(g, &st, &ct);
                diff = sp * ct - cp * st;
                jac = cp * ct + sp * st;
            }
            const float cwk = d.code_weights[k];
            const float dw = cwk * diff, ad = fabsf(dw);
            const bool lt = ad <= knee;
            const float as = ad * d.sigma;
            const float l = (lt ? 0.5f * (as * as) : ad - half_knee) * rw;
            const float dl = lt ? s2 * dw : (dw > 0.f ? 1.f : -1.f);
            s_box[t * 7 + k] = gloc * rw * dl * cwk * jac;
            s_tgt[t * 7 + k] = l;
            sum_loc += l;
        }

        // direction: two-way softmax cross-entropy = softplus(other logit - target logit) (losses.py:387-391), weights [label > 0] / max(numpos, 1)
        if (d.has_dir) {
            const float rot = tgt6 + anc6;                                     // the float32 sum (:579)
            const bool up = rot > 0.f;                                         // target class 1
            float sg, sgn, l1p;
            const float u = up ? lg.x - lg.y : lg.y - lg.x;
            dl_sigmoids(u, sg, sgn, l1p);
            const float l = (fmaxf(u, 0.f) + l1p) * rw;
            const float go = d.dir_weight / fB * rw * sg;                    // gradient at the other logit; the target's is its negative
            reinterpret_cast<float2 *>(a.io.ddir)[base + t] = up ? make_float2(go, -go) : make_float2(-go, go);
            sum_dir = l;
        }
    }
    __syncthreads();
    // flat, coalesced stores
    {
        float *gb = a.io.dbox + base * 7, *gl = a.io.loc_loss ? a.io.loc_loss + base * 7 : nullptr;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int i = t + DL_T * j;
            if (i < nv * 7) { gb[i] = s_box[i]; if (gl) gl[i] = s_tgt[i]; }
        }
        float *gc = a.io.dcls + base * C, *gcl = a.io.cls_loss ? a.io.cls_loss + base * C : nullptr;
        for (int i = t; i < nv * C; i += DL_T) {
            const int o = (i / C) * Cp + i % C;
            gc[i] = s_cls[o];
            if (gcl) gcl[i] = s_cl2[o];
        }
    }
    // the workgroup's five sums: lanes in the DPP order of wave_sum_f32_to_lane63, then the four waves in order
    const float v[5] = {sum_loc, sum_cls, sum_dir, sum_pos, sum_neg};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float s = wave_sum_f32_to_lane63(v[j]);
        if (lane_id() == 63) s_red[t >> 6][j] = s;
    }
    __syncthreads();
    if (t < DL_SLOTS) a.part[(int64_t)w * DL_SLOTS + t] = t < 5 ? ((s_red[0][t] + s_red[1][t]) + s_red[2][t]) + s_red[3][t] : 0.f;
}

__global__ __launch_bounds__(1024) void dl_fold_kernel(const DlArgs a)
{
    __shared__ float red[16][64];
    __shared__ float s_tot[64], s_fin[DL_SLOTS];
    const int el = threadIdx.x & 63;
    float s;
    if (fold_lanes<16, 8>(a.part, 64, a.nchunks, el, true, red, s)) s_tot[el] = s;
    __syncthreads();
    if (threadIdx.x < DL_SLOTS) {
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < DL_ROWS_PER_CHUNK; ++g) v += s_tot[g * DL_SLOTS + threadIdx.x];
        s_fin[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const papc_det_loss_desc &d = a.d;
        const float fB = (float)d.B;
        const float loc = s_fin[0] / fB * d.loc_weight, cls = s_fin[1] / fB * d.cls_weight, dir = s_fin[2] / fB;      // (:181-187, :198)
        float loss = loc + cls;
        if (d.has_dir) loss += dir * d.dir_weight;
        float *o = a.io.out;
        o[0] = loss; o[1] = loc; o[2] = cls; o[3] = dir;
        o[4] = s_fin[3] / fB / d.pos_cls_weight;                                                                     // (:183-185)
        o[5] = s_fin[4] / fB / d.neg_cls_weight;
        o[6] = 0.f; o[7] = 0.f;
    }
}

static int dl_check_desc(const char *who, const papc_det_loss_desc *d)
{
    PAPC_REQUIRE(d, PAPC_E_INVALID, "%s: null descriptor", who);
    PAPC_REQUIRE(d->B >= 1 && d->B <= 65535 && d->A >= 1 && d->C >= 1 && (int64_t)d->B * d->A <= ((int64_t)1 << 28), PAPC_E_INVALID,
                 "%s: B=%d A=%d C=%d out of range (B in 1..65535, A >= 1, C >= 1, B * A <= 2^28)", who, d->B, d->A, d->C);
    PAPC_REQUIRE(d->norm_type >= 0 && d->norm_type <= 2, PAPC_E_INVALID, "%s: norm_type=%d is not one of PAPC_DET_NORM_*", who, d->norm_type);
    PAPC_REQUIRE(d->sigma > 0.f && d->gamma >= 0.f, PAPC_E_INVALID, "%s: sigma=%g must be > 0 and gamma=%g >= 0", who, d->sigma, d->gamma);
    PAPC_REQUIRE(d->C <= DL_CMAX, PAPC_E_UNSUPPORTED, "%s: C=%d classes > %d", who, d->C, DL_CMAX);
    PAPC_REQUIRE(d->code_size == 7, PAPC_E_UNSUPPORTED, "%s: box code size %d (the kernels are built for 7)", who, d->code_size);
    PAPC_REQUIRE(d->encode_background_as_zeros != 0, PAPC_E_UNSUPPORTED, "%s: encode_background_as_zeros = False is not built", who);
    PAPC_REQUIRE(d->codewise != 0, PAPC_E_UNSUPPORTED, "%s: non-codewise smooth L1 is not built", who);
    return PAPC_OK;
}

// the launch geometry and the workspace: [counts 2 B, count partials 2 B ncb (one piece) | partial rows]
static size_t dl_layout(const papc_det_loss_desc *d, void *base, DlArgs &a)
{
    a.nblk = (int)cdiv(d->A, DL_T);
    a.ncb = (int)cdiv(d->A, DL_CNT);
    a.nrows = d->B * a.nblk;
    a.nchunks = (int)cdiv(a.nrows, DL_ROWS_PER_CHUNK);
    WsCarver c{static_cast<char *>(base), 0, 16};
    a.counts = c.take<int32_t>(2 * (size_t)d->B + 2 * (size_t)d->B * a.ncb);
    a.cnt_part = base ? a.counts + 2 * (int64_t)d->B : nullptr;
    a.part = c.take<float>((size_t)a.nchunks * 64);
    return c.off;
}

}  // namespace papc

using namespace papc;

extern "C" int papc_det_loss_workspace(const papc_det_loss_desc *desc, int64_t *bytes)
{
    int rc = dl_check_desc("papc_det_loss_workspace", desc);
    if (rc) return rc;
    PAPC_REQUIRE(bytes, PAPC_E_INVALID, "papc_det_loss_workspace: null pointer");
    DlArgs a;
    *bytes = (int64_t)dl_layout(desc, nullptr, a);
    return PAPC_OK;
}

extern "C" int papc_det_loss_fwd_f32(const papc_det_loss_desc *desc, const papc_det_loss_io *io, papc_stream_t stream)
{
    const char *who = "papc_det_loss_fwd_f32";
    int rc = dl_check_desc(who, desc);
    if (rc) return rc;
    PAPC_REQUIRE(io, PAPC_E_INVALID, "%s: null io", who);
    PAPC_REQUIRE(io->box_preds && io->cls_preds && io->labels && io->reg_targets, PAPC_E_INVALID, "%s: null input pointer", who);
    PAPC_REQUIRE(io->out && io->dbox && io->dcls && io->workspace, PAPC_E_INVALID, "%s: null output or workspace pointer", who);
    if (desc->has_dir) {
        PAPC_REQUIRE(io->dir_preds && io->anchors && io->ddir, PAPC_E_INVALID, "%s: null direction pointer (dir_preds, anchors, ddir) with has_dir", who);
        PAPC_REQUIRE((reinterpret_cast<uintptr_t>(io->dir_preds) & 7) == 0 && (reinterpret_cast<uintptr_t>(io->ddir) & 7) == 0, PAPC_E_INVALID,
                     "%s: dir_preds and ddir must be 8-byte aligned", who);
    }
    PAPC_REQUIRE(aligned16(io->workspace), PAPC_E_INVALID, "%s: workspace must be 16-byte aligned", who);
    DlArgs a;
    memset(&a, 0, sizeof(a));
    a.d = *desc;
    a.io = *io;
    dl_layout(desc, io->workspace, a);
    hipStream_t st = as_stream(stream);
    const dim3 cgrid((unsigned)a.ncb, (unsigned)desc->B);
    const unsigned mgrid = (unsigned)a.nchunks * DL_ROWS_PER_CHUNK;
    const size_t mlds = 2 * (size_t)DL_T * (desc->C | 1) * sizeof(float);
    if (desc->labels_i64) {
        hipLaunchKernelGGL(dl_count_kernel<int64_t>, cgrid, dim3(256), 0, st, static_cast<const int64_t *>(io->labels), desc->A, a.ncb, a.cnt_part, io->cared);
        hipLaunchKernelGGL(dl_main_kernel<int64_t>, dim3(mgrid), dim3(DL_T), mlds, st, a);
    } else {
        hipLaunchKernelGGL(dl_count_kernel<int32_t>, cgrid, dim3(256), 0, st, static_cast<const int32_t *>(io->labels), desc->A, a.ncb, a.cnt_part, io->cared);
        hipLaunchKernelGGL(dl_main_kernel<int32_t>, dim3(mgrid), dim3(DL_T), mlds, st, a);
    }
    hipLaunchKernelGGL(dl_fold_kernel, dim3(1), dim3(1024), 0, st, a);
    return check_launch(who);
}
