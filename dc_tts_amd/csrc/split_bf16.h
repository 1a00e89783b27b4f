// split_bf16.h -- fp32 -> bf16 term splits shared by the inference contraction (hconv_kernel.h, split behind the LDS read) and the
// training GEMM (train_gemm3_kernel.h, split in front of the LDS store).  Device inline functions only: any translation unit may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dctts {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

// Split-bf16 contraction (round 5, OPT-IN: dctts_set_split_bf16; the default and the headline stay exact fp32).  A float is written as two bf16 terms,
// x = hi + mid + r with hi = bf16(x), mid = bf16(x - hi) (both round-to-nearest: v_cvt_pk_bf16_f32; x - hi is exact) and |r| <= 2^-18 |x|, and a product is
// accumulated in fp32 from three matrix instructions  hi.hi + hi.mid + mid.hi  (what is dropped, mid.mid and the r terms, is <= 2^-16 of |x||w|), on
// v_mfma_f32_32x32x16_bf16 at 16x the fp32 matrix rate: 3 x 32 cycles per 16 k against 8 x 64.  The weights are split once at upload, the activations in
// registers behind the LDS read.  Two packed halves of a pair (x0, x1) -> their (hi, mid) words:
__device__ __forceinline__ void split_bf16_pair(float x0, float x1, unsigned& hi, unsigned& mid) {
  const bf16x2_t h = __builtin_convertvector((f32x2_t){x0, x1}, bf16x2_t);
  hi = __builtin_bit_cast(unsigned, h);
  const float h0 = __uint_as_float(hi << 16), h1 = __uint_as_float(hi & 0xffff0000u);
  const bf16x2_t m = __builtin_convertvector((f32x2_t){x0 - h0, x1 - h1}, bf16x2_t);
  mid = __builtin_bit_cast(unsigned, m);
}
// Three-term split (opt-in: dctts_set_split_bf16_terms(ctx, 3); hconv_kernel<BF = 2>).  x = hi + mid + lo EXACTLY: x - hi has at most 16 significant bits, mid takes the
// upper 8 of them, so lo = bf16(x - hi - mid) is exact as well (both subtractions are exact in fp32; only a remainder below the bf16 subnormal range is lost).  Six
// products are accumulated, small terms first:  lo.hi + hi.lo + mid.mid + mid.hi + hi.mid + hi.hi;  what is dropped, mid.lo + lo.mid + lo.lo, is <= ~2^-26 of |x||w|
// per product -- below one fp32 accumulate rounding (2^-24) -- and the accumulator is rounded 6 times per 16 k where the fp32 instruction rounds it 8 times.
// 6 x 32 matrix cycles per 16 k against 3 x 32 (two terms) and 8 x 64 (fp32).
// (The four subtractions are single v_sub_f32: written out so that the pairs are never fused into packed fp32 instructions.)
__device__ __forceinline__ float split_sub_f32(float a, float b) { float d; asm("v_sub_f32_e32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ void split_bf16_pair3(float x0, float x1, unsigned& hi, unsigned& mid, unsigned& lo) {
  const bf16x2_t h = __builtin_convertvector((f32x2_t){x0, x1}, bf16x2_t);
  hi = __builtin_bit_cast(unsigned, h);
  const float r0 = split_sub_f32(x0, __uint_as_float(hi << 16)), r1 = split_sub_f32(x1, __uint_as_float(hi & 0xffff0000u));
  const bf16x2_t m = __builtin_convertvector((f32x2_t){r0, r1}, bf16x2_t);
  mid = __builtin_bit_cast(unsigned, m);
  const bf16x2_t l = __builtin_convertvector((f32x2_t){split_sub_f32(r0, __uint_as_float(mid << 16)), split_sub_f32(r1, __uint_as_float(mid & 0xffff0000u))}, bf16x2_t);
  lo = __builtin_bit_cast(unsigned, l);
}

}  // namespace dctts
