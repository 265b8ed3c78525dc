// The MXFP8 (e4m3 + e8m0) quantizer and its inverse, in one place so that
// the scale rule, the 2^-126 clamp and the cvt_pk_fp8_f32 rounding cannot
// drift apart.  Users:
//
//   mx_gemm.hip        mx_quantize_rows_kernel   one thread per 32-block
//   decode_attn_mx.hip mx_kv_store_kernel        one thread per 32-block
//                      damx_append_block         the same, from LDS, + dequant
//                      decode_attn_mx_part       dequant of cache rows
//   chunk_attn.hip     chunk_attn_append         one thread per 32-block
//                      chunk_attn_part           dequant of a tile into LDS
//   mx_skinny.hip      the fused quantizer: one lane per 16-element half
//                      block, in the MFMA's operand layout
//
// The four pieces:
//
//   ab  = mxq_amax_bits(...)   block amax on the bf16 magnitude bits
//   e   = mxq_block_exp(ab)    smallest e with amax * 2^-e <= 448, clamped
//   inv = mxq_inv_scale(e)     2^-e, exact
//   mxq_cvt8(v, inv, w0, w1)   8 bf16 -> 8 e4m3 bytes in memory order
//
// mxq_block32 chains them for one whole block held by one thread; the
// half-block mapping of mx_skinny.hip calls the pieces itself.  The inverse
// is mxq_scale (e8m0 byte -> float) and mxq_dcvt8 (8 e4m3 bytes -> floats).
//
// Bit-identical to pack_mx(*quantize_mx(x, "fp8_e4m3")) of
// quantization/microscaling.py (tests/test_mx_gemm_gpu.py::test_quantize_*).
#pragma once

#include "common.h"

typedef unsigned int uint4v __attribute__((ext_vector_type(4)));
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));

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

// One 32-element block held as four s8v: the 32 e4m3 bytes in memory order
// into out[0..1]; returns the block exponent e (the scale byte is e + 127).
__device__ __forceinline__ int mxq_block32(const s8v* v, uint4v* out) {
  int ab = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) ab = mxq_amax_bits(v[i], ab);
  const int e = mxq_block_exp(ab);
  const float inv = mxq_inv_scale(e);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned w0, w1;
    mxq_cvt8(v[i], inv, w0, w1);
    out[i >> 1][2 * (i & 1)] = w0;
    out[i >> 1][2 * (i & 1) + 1] = w1;
  }
  return e;
}

// The inverse.  Scale byte b in 1..254 is 2^(b-127), built as the float with
// exponent field b; byte 0 (all-zero / negligible block) reads as 0.
__device__ __forceinline__ float mxq_scale(unsigned b) {
  union { unsigned u; float f; } c;
  c.u = b << 23;
  return c.f;
}

// 8 e4m3 bytes in memory order -> 8 floats (v_cvt_pk_f32_fp8)
__device__ __forceinline__ void mxq_dcvt8(uint2v w, float* f) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f2v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f2v hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}
