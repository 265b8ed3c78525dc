// The MXFP8 (e4m3 + e8m0) activation quantizer, shared by mx_quantize_rows
// (mx_gemm.hip: one thread per 32-element block) and the fused quantizer of
// mx_skinny.hip (one lane per 16-element half block, in the MFMA's operand
// layout).  Both are built from the same four pieces, so the scale rule, the
// 2^-126 clamp and the cvt_pk_fp8_f32 rounding cannot drift apart:
//
//   ab  = mxq_amax_bits(...)   block amax on the bf16 magnitude bits
//   e   = mxq_block_exp(ab)    smallest e with amax * 2^-e <= 448, clamped
//   inv = mxq_inv_scale(e)     2^-e, exact
//   mxq_cvt8(v, inv, w0, w1)   8 bf16 -> 8 e4m3 bytes in memory order
//
// Bit-identical to pack_mx(*quantize_mx(x, "fp8_e4m3")) of
// quantization/microscaling.py (tests/test_mx_gemm_gpu.py::test_quantize_*).
#pragma once

#include "common.h"

// running max of the bf16 magnitude bits (ordered like the values)
__device__ __forceinline__ int mxq_amax_bits(s8v v, int ab) {
#pragma unroll
  for (int j = 0; j < 8; ++j) ab = max(ab, (int)v[j] & 0x7FFF);
  return ab;
}

// block exponent from the block's amax bits; the biased e8m0 byte is e + 127
__device__ __forceinline__ int mxq_block_exp(int ab) {
  ab = max(ab, 0x0080);  // clamp to 2^-126 (zero / subnormal block)
  // smallest e with amax * 2^-e <= 448 = 1.75 * 2^8, amax = 1.m * 2^E
  const int E = (ab >> 7) - 127;
  const int e = E - 8 + ((ab & 0x7F) > 0x60 ? 1 : 0);
  return min(max(e, -127), 127);
}

__device__ __forceinline__ float mxq_inv_scale(int e) {
  union { unsigned u; float f; } inv;
  inv.u = (unsigned)(127 - e) << 23;  // 2^-e, exact (e <= 121)
  return inv.f;
}

// elements 0..3 -> bytes 0..3 of w0, elements 4..7 -> bytes 0..3 of w1
__device__ __forceinline__ void mxq_cvt8(s8v v, float inv, unsigned& w0,
                                         unsigned& w1) {
  int a = 0, b = 0;
  a = __builtin_amdgcn_cvt_pk_fp8_f32(bits2f(v[0]) * inv, bits2f(v[1]) * inv,
                                      a, false);
  a = __builtin_amdgcn_cvt_pk_fp8_f32(bits2f(v[2]) * inv, bits2f(v[3]) * inv,
                                      a, true);
  b = __builtin_amdgcn_cvt_pk_fp8_f32(bits2f(v[4]) * inv, bits2f(v[5]) * inv,
                                      b, false);
  b = __builtin_amdgcn_cvt_pk_fp8_f32(bits2f(v[6]) * inv, bits2f(v[7]) * inv,
                                      b, true);
  w0 = (unsigned)a;
  w1 = (unsigned)b;
}
