// Split-operand MFMA helpers: float32-accurate products on the bf16 / fp16 matrix cores.  Shared by the radial MLP
// (radial_mlp.hip, radial_mlp_pipe.h), the node linear maps (node_ops.hip, node_fused.h) and the weight gradients
// (wgrad.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nqa {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// ---- three-plane bf16 split ("bf16x6") --------------------------------------------------------------------------------
// Every fp32 operand is written as the exact sum of three bf16 numbers, x = hi + mid + lo (8 + 8 + 8 significand
// bits; the residuals are formed exactly in fp32), and a product is accumulated in fp32 from the six partial
// products whose weight is >= 2^-16:  hi.hi + hi.mid + mid.hi + (mid.mid + hi.lo + lo.hi).  The dropped terms
// (mid.lo, lo.mid, lo.lo) are below 2^-24 relative -- the rounding level of an fp32 fma chain -- so the result
// carries fp32 accuracy (tests/test_radial_mlp.py measures both variants against float64), while
// v_mfma_f32_32x32x16_bf16 retires 16x the MACs per cycle of v_mfma_f32_32x32x2_f32: 6 instructions of 16384 MACs
// replace 8 of 2048 for the same tile, i.e. 2.7x the fp32-MFMA ceiling.
//
// v_mfma_f32_32x32x16_bf16 register maps: A: lane l holds A[i = l&31][k = 8*(l>>5) + t], t = 0..7 (4 VGPRs);
// B: B[k = 8*(l>>5) + t][j = l&31]; D as the 32x32 fp32 form.
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));  // round-to-nearest-even, lo -> bits [15:0]
  return r;
}

// two floats -> three packed bf16 pairs with x == hi + mid + lo (+ O(2^-25))
__device__ __forceinline__ void split_pair(float x0, float x1, uint32_t& h, uint32_t& m, uint32_t& l) {
  h = cvt_pk_bf16(x0, x1);
  float r0 = x0 - __uint_as_float(h << 16);
  float r1 = x1 - __uint_as_float(h & 0xffff0000u);
  m = cvt_pk_bf16(r0, r1);
  r0 -= __uint_as_float(m << 16);
  r1 -= __uint_as_float(m & 0xffff0000u);
  l = cvt_pk_bf16(r0, r1);
}

__device__ __forceinline__ f32x16 mfma_bf16(const u32x4& a, const u32x4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                 0);
}

// ---- two-plane fp16 split ("f16x3"): x = h + l with h = fp16(x), l = fp16(x - h) represents x to 2^-22 |x| (two
// 11-bit significands), so a product needs three matrix instructions (h h, h l, l h; the dropped l l term is 2^-24 of
// the product) accumulated into ONE fp32 accumulator, instead of the six of the three-plane bf16 split.  fp16 has no
// exponent range to spare, so every operand is first multiplied by a power of two that puts the largest magnitude of its
// group into [2^14, 2^15) -- exact, undone on the accumulators.  With the group's maximum up there, whatever falls
// below fp16's smallest normal number 2^-14 -- an element under 2^-28 of the maximum, or the low part of an element
// under 2^-17 of it -- is lost to at most 2^-14 absolute = 2^-28 of the maximum, whether or not the matrix pipe flushes
// subnormal inputs.
__device__ __forceinline__ f32x16 mfma_f16(const u32x4& a, const u32x4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ void split_pair_f16(float x0, float x1, uint32_t& h, uint32_t& l) {
  const f16x2 hh = {(_Float16)x0, (_Float16)x1};
  const f16x2 ll = {(_Float16)(x0 - (float)hh[0]), (_Float16)(x1 - (float)hh[1])};
  h = __builtin_bit_cast(uint32_t, hh);
  l = __builtin_bit_cast(uint32_t, ll);
}

// power of two that brings a maximum magnitude m into [2^14, 2^15); 1 for m = 0 or a non-finite m (the row / tile then
// carries its inf / NaN through the fp16 conversion as the fp32 arithmetic would)
__device__ __forceinline__ float f16_scale_up(float m) {
  if (!(m > 0.f) || !(m < 3.0e38f)) return 1.f;
  int e;
  (void)frexpf(m, &e);  // m = f 2^e, f in [0.5, 1)
  int k = 15 - e;
  k = k > 100 ? 100 : (k < -100 ? -100 : k);
  return ldexpf(1.f, k);
}

}  // namespace nqa
