// The quantize-and-append of one new row for the one-token kernels over an
// MXFP8 KV cache: decode_attn_mx.hip (dense cache) and paged_attn_mx.hip
// (pages).  The row lies in LDS as bf16 bits; the caller hands in the
// addresses of the cache row's payload and scale bytes.
#pragma once

#include "mx_quant.h"

// One thread quantizes the 32-element block `blk` of a 128-wide bf16 row held
// in LDS, writes payload + scale byte to the cache row and the dequantized
// values back to LDS.
__device__ __forceinline__ void damx_append_block(
    const short* __restrict__ row_bits, int blk, uint8_t* __restrict__ payload,
    uint8_t* __restrict__ scales, float* __restrict__ deq) {
  s8v v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) v[i][j] = row_bits[32 * blk + 8 * i + j];
  uint4v out[2];
  const int e = mxq_block32(v, out);
  const float sc = mxq_scale((unsigned)(e + 127));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float f[8];
    mxq_dcvt8(uint2v{out[i >> 1][2 * (i & 1)], out[i >> 1][2 * (i & 1) + 1]},
              f);
#pragma unroll
    for (int j = 0; j < 8; ++j) deq[32 * blk + 8 * i + j] = f[j] * sc;
  }
  uint4v* dst = (uint4v*)(payload + 32 * blk);
  dst[0] = out[0];
  dst[1] = out[1];
  scales[blk] = (uint8_t)(e + 127);
}
