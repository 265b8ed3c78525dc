// The 8 KiB LDS image of one TRANSPOSED 64x64 bf16 tile, shared by
// transpose.hip and the dual-output SwiGLU backward (swiglu.hip).  Layout,
// chunk swizzle and the banking argument: transpose.hip's header comment and
// profiles/KERNEL_NOTES.md, "Backward GEMM layout".
//
// 64 rows (source column c) of 32 dwords; dword d of row c holds
// src[2d][c] | src[2d+1][c] << 16; 16-byte chunk k of row c is kept at chunk
// k ^ ((c>>3)&7).
#pragma once

#include "common.h"

typedef unsigned u4v __attribute__((ext_vector_type(4)));

#define TR_TILE 64
#define TR_IMAGE_DWORDS (TR_TILE * 32)

// Thread (chunk ch = 8 source columns, row pair rp) stores its two 16-byte
// row pieces a (row 2rp) and b (row 2rp+1): 8 ds_write_b32, one per column.
__device__ __forceinline__ void tr_image_put(unsigned* tile, int ch, int rp,
                                             u4v a, u4v b) {
  unsigned* w = tile + (8 * ch) * 32 + (rp ^ (ch << 2));
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[(2 * k) * 32] = (a[k] & 0xffffu) | (b[k] << 16);
    w[(2 * k + 1) * 32] = (a[k] >> 16) | (b[k] & 0xffff0000u);
  }
}

// Source rows 8q..8q+7 of source column cl: one ds_read_b128.
__device__ __forceinline__ u4v tr_image_get(const unsigned* tile, int cl,
                                            int q) {
  return *(const u4v*)(tile + cl * 32 + ((q ^ ((cl >> 3) & 7)) << 2));
}
