// Element-level arithmetic of the table's row formats: what turns one fp32 value (and its row's / group's / block's maximum)
// into stored bits.  Shared by the two kernels that write table rows from fp32 -- k_store_f32 (scone_table.hip) and k_opt_step
// (scone_opt.hip) -- which differ only in how lanes map to elements; the maxima are exact, so the mapping cannot show in the bits.
// The numpy statements: oracle/ref_port.py quantize_i8 / quantize_i4, tests/bf16_fixture.py to_bf16_bits, tests/mxfp4_fixture.py
// quantize (the formats themselves: include/scone_hip.h).
#pragma once

#include "scone_common.h"

// fp32 -> bfloat16 bits, IEEE round-to-nearest-even: a tie (low half 0x8000) goes to the even upper half, a finite value
// beyond the largest bf16 carries into the exponent and becomes +-inf, fp32 subnormals round into bf16 subnormals, -0.0 and
// +-inf pass through.  NaN is taken out first: the increment would carry a NaN with a high payload into the sign bit
// (0x7FFFFFFF -> 0x8000 = -0.0) and a truncation could leave the infinity's 0x7F80; it stays a NaN with the quiet bit set.
__device__ __forceinline__ unsigned short scone_f32_to_bf16_bits(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (unsigned short)((u >> 16) | 0x0040u);
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// the maximum over the wave's 64 lanes, in every lane (exact: no rounding, so the lane mapping cannot show)
__device__ __forceinline__ float scone_wave_max(float v) {
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}

// INT8 (qmax = 127, amax over the row) and INT4 (qmax = 7, amax over a group of 128): the fp16 scale, and the integer of one
// element as a float in [-qmax, qmax] (0 where the scale is 0 -- or NaN: the comparison is false)
__device__ __forceinline__ __half scone_q_scale(float amax, float qmax) { return __float2half_rn(amax / qmax); }
__device__ __forceinline__ float scone_q_elem(float x, float sf, float qmax) {
  float q = 0.f;
  if (sf > 0.f) q = fminf(fmaxf(rintf(x / sf), -qmax), qmax);
  return q;
}

// MXFP4, OCP MX v1.0.  The E8M0 scale of a block from the largest |bits| in it: a NaN / inf in the block -> X = 255; else
// X = max(0, exponent field of amax - 2) (amax = 0: 127), which is clamp(floor(log2 amax) - 2 + 127, 0, 254) -- a subnormal amax
// has field 0, FLT_MAX 254 -> 252.
__device__ __forceinline__ uint32_t scone_mx_block_scale(uint32_t amax_bits) {
  return amax_bits >= 0x7F800000u ? 255u : (amax_bits == 0u ? 127u : ((amax_bits >> 23) > 2u ? (amax_bits >> 23) - 2u : 0u));
}
// The E2M1 nibble of one element (its fp32 bits) under scale X.  q = |v| 2^(127-X) is exact (a power-of-two scaling; where it
// underflows it is far below the first midpoint), and the comparisons are round-to-nearest with ties to the even code:
// 0.25 -> 0, 0.75 -> 1.0, 1.25 -> 1.0, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4.
__device__ __forceinline__ uint32_t scone_mx_nibble(uint32_t bits, uint32_t X) {
  uint32_t code = 0;
  if (X != 255u) {
    const float q = __uint_as_float(bits & 0x7FFFFFFFu) * __uint_as_float((254u - X) << 23);
    code = (q > 0.25f) + (q >= 0.75f) + (q > 1.25f) + (q >= 1.75f) + (q > 2.5f) + (q >= 3.5f) + (q > 5.0f);
  }
  return code | ((bits >> 31) << 3);
}
