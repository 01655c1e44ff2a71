// bf16x3.h -- fp32 on the bf16 matrix pipe: the exact 3-way split and its six-product order, written once.
//
// x = x1 + x2 + x3 with x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2) (round-to-nearest-even each; the
// subtractions are exact in fp32).  Three 8-bit significands cover the 24-bit fp32 significand, so the split is exact
// (up to underflow of the tails), and a product a*b is recovered as the six bf16 products
//   a1*b1 + (a1*b2 + a2*b1) + (a1*b3 + a2*b2 + a3*b1)
// accumulated in fp32 by v_mfma_f32_32x32x16_bf16; the dropped terms (a2*b3, a3*b2, a3*b3) are below 2^-26 |a*b|,
// i.e. under the rounding error of a single fp32 multiply-add.  6 MFMAs of 32 cycles per 32x32x16 block against
// 8 x 64 cycles of v_mfma_f32_32x32x2_f32 for the same block: 2.7x the fp32 matrix rate at fp32 accuracy
// (tools/probe/mfma_bf16_layout.hip measures 6.5e-8 max |err| / sum|a_k b_k| vs 1.5e-7 for the fp32 fma chain).
// An accumulator receives its six products smallest terms first: a3b1, a2b2, a1b3, a2b1, a1b2, a1b1 (BF16X3_PA / BF16X3_PB).
// Both the split and that order are part of what makes a training step bit-reproducible: every MFMA body takes them from
// here (tests/test_gpu_bf16x3.py pins the split bit for bit).
#pragma once
#include "common.h"

namespace papc {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float floatx2_t __attribute__((ext_vector_type(2)));
typedef float floatx16 __attribute__((ext_vector_type(16)));   // the 32x32 accumulator

__device__ __forceinline__ unsigned pack_bf16x2(float a, float b)  // -> v_cvt_pk_bf16_f32 (a in the low half)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((floatx2_t){a, b}, bf16x2_t));
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

#ifndef PAPC_SPLIT_PK
#define PAPC_SPLIT_PK 0   // 1: the two exact subtractions of a pair as one v_pk_add_f32 -- measured SLOWER in the LDS-staged kernels (dW family 0.85 -> 0.90 ms/step: the producers pay moves to form aligned register pairs); the row-streaming kernel, whose pairs are natural, uses split3_pair
#endif
// one level of the split of four consecutive-k values: the leading bf16 of each value (4 packed bf16, 8 bytes), and what is left
__device__ __forceinline__ void split_level(float4 &r, uint2 &pl)
{
    pl.x = pack_bf16x2(r.x, r.y); pl.y = pack_bf16x2(r.z, r.w);
#if PAPC_SPLIT_PK
    const floatx2_t a = floatx2_t{r.x, r.y} - floatx2_t{bf16_lo(pl.x), bf16_hi(pl.x)}, b = floatx2_t{r.z, r.w} - floatx2_t{bf16_lo(pl.y), bf16_hi(pl.y)};
    r = make_float4(a.x, a.y, b.x, b.y);
#else
    r.x -= bf16_lo(pl.x); r.y -= bf16_hi(pl.x); r.z -= bf16_lo(pl.y); r.w -= bf16_hi(pl.y);
#endif
}
// planes p0 (leading), p1, p2 of four consecutive-k values (what is left after the third level is dropped)
__device__ __forceinline__ void split3(float4 v, uint2 &p0, uint2 &p1, uint2 &p2)
{
    split_level(v, p0); split_level(v, p1); split_level(v, p2);
}
// ... of one pair (consecutive k as a 64-bit register pair: the subtractions are one v_pk_add_f32 each)
__device__ __forceinline__ void split3_pair(floatx2_t x, unsigned &p0, unsigned &p1, unsigned &p2)
{
    p0 = pack_bf16x2(x.x, x.y);
    x = x - floatx2_t{bf16_lo(p0), bf16_hi(p0)};
    p1 = pack_bf16x2(x.x, x.y);
    x = x - floatx2_t{bf16_lo(p1), bf16_hi(p1)};
    p2 = pack_bf16x2(x.x, x.y);
}
// ... of eight consecutive-k values, as the three operand fragments of a lane of v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8 (&pl)[3])
{
    uint2 a0, a1, a2, b0, b1, b2;
    split3(make_float4(v[0], v[1], v[2], v[3]), a0, a1, a2);
    split3(make_float4(v[4], v[5], v[6], v[7]), b0, b1, b2);
    pl[0] = __builtin_bit_cast(bf16x8, make_uint4(a0.x, a0.y, b0.x, b0.y));
    pl[1] = __builtin_bit_cast(bf16x8, make_uint4(a1.x, a1.y, b1.x, b1.y));
    pl[2] = __builtin_bit_cast(bf16x8, make_uint4(a2.x, a2.y, b2.x, b2.y));
}

// product t of an accumulator is a[BF16X3_PA[t]] * b[BF16X3_PB[t]]
constexpr int BF16X3_PA[6] = {2, 1, 0, 1, 0, 0}, BF16X3_PB[6] = {0, 1, 2, 0, 1, 0};

// acc + a * b: the six issues of one 32x32x16 block back to back (kernels that interleave several accumulators index the table themselves)
__device__ __forceinline__ floatx16 mfma_bf16x3(const bf16x8 (&a)[3], const bf16x8 (&b)[3], floatx16 acc)
{
#pragma unroll
    for (int t = 0; t < 6; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[BF16X3_PA[t]], b[BF16X3_PB[t]], acc, 0, 0, 0);
    return acc;
}

}  // namespace papc
