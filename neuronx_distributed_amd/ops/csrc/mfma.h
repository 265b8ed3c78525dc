// MFMA fragment helpers for v_mfma_f32_32x32x16_bf16 on gfx950.
//
// Layout contracts (verified by tests/test_ops_gpu.py numerics on MI355X):
//   A operand (32x32x16): lane l supplies A[m = l&31][k = 8*(l>>5) + j], j=0..7
//   B operand:            lane l supplies B[k = 8*(l>>5) + j][n = l&31]
//   C/D accumulator (16 f32/lane): element r holds
//       row m = (r&3) + 8*(r>>2) + 4*(l>>5),  col n = l&31
// (cdna_hip_programming.md §3 Fragment layout.)
#pragma once

#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int uint4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

union frag_u {
  bf16x8 bf;
  uint4v u4;
  uint u[4];
};

// accumulator row index for C/D element r (lane-half hi = lane>>5)
__device__ __forceinline__ int acc_row(int r, int hi) {
  return (r & 3) + 8 * (r >> 2) + 4 * hi;
}

// pack two f32 into one u32 of 2 bf16: use the compiler's native casts so
// it can emit v_cvt_pk_bf16_f32 (a hand-rolled RNE costs ~5 VALU per pair,
// cdna_hip_programming.md T12)
__device__ __forceinline__ uint pack_bf16x2(float lo, float hi) {
  union { __bf16 b[2]; uint u; } r;
  r.b[0] = (__bf16)lo;
  r.b[1] = (__bf16)hi;
  return r.u;
}

// ---------------------------------------------------------------------------
// Dual-use LDS image of a [rows][128 bf16] tile (cdna_hip_programming.md
// T10, layout (b)): plain 256-byte rows whose 16-byte chunks are XORed so
// that ONE copy serves both the ds_read_b128 row read (A operand, row =
// lane) and the ds_read_b64_tr_b16 transposed read (B operand, column =
// lane) of the 32x32x16 mfma without bank conflicts.  Every store and every
// read goes through img_off(); tests/test_flash_bwd_pipeline_gpu.py checks
// the complete fragment maps on the GPU (probe_lds_image.hip).
// ---------------------------------------------------------------------------
#define IMG_ROW_B 256

// byte offset of 16-byte chunk ch (0..15) of row `row`
__device__ __forceinline__ int img_off(int row, int ch) {
  return IMG_ROW_B * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// The XOR only touches byte bits 4..7, so for both kinds of read the
// lane-dependent part of the address is ONE base register: the chunk / row
// block / column block selected by compile-time indices enters as an XOR
// with a constant < 256 plus a constant multiple of 256, and any tile or
// buffer offset that is a multiple of 256 may be pre-added to the base.

// A-operand row read: lane supplies X[row][16*c + 8*hi + j], j = 0..7.
// base = img_row_base(row, hi) [+ 256-aligned offsets]
__device__ __forceinline__ int img_row_base(int row, int hi) {
  return img_off(row, hi);
}
__device__ __forceinline__ uint4v img_row_read(const char* img, int base,
                                               int c) {
  return *(const uint4v*)(img + (base ^ (32 * c)));
}

// B-operand transposed read: lane l supplies X[k0 + 8*(l>>5) + j][n0 +
// (l&31)], j = 0..7, for a k-block k0 (multiple of 16) and a column block
// n0 (multiple of 32).  Two ds_read_b64_tr_b16, one per 4 k rows; each
// 16-lane group reads a 4-row x 16-column block, lane 4q+p of the group
// addressing row q, columns 4p..4p+3 (8 bytes of one chunk, 8-byte
// aligned).  base = img_tr_base(lane) [+ 256-aligned offsets].
// EXEC must be all ones here: call only under wave-uniform control flow.
typedef short s4v_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int img_tr_base(int lane) {
  const int i = lane & 15;
  const int q = i >> 2, p = i & 3;
  return img_off(8 * (lane >> 5) + q, 2 * ((lane >> 4) & 1) + (p >> 1)) +
         8 * (p & 1);
}
__device__ __forceinline__ uint4v img_tr_read(const char* img, int base,
                                              int k0, int n0) {
  typedef __attribute__((address_space(3))) s4v_t lds_s4v;
  union { s4v_t s[2]; uint4v u4; } r;
  // rows k0+8hi+q: chunk XOR term as in base; rows +4: its bit 0 flips
  r.s[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s4v*)(img + (base ^ (2 * n0)) + IMG_ROW_B * k0));
  r.s[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s4v*)(img + (base ^ (2 * n0) ^ 16) + IMG_ROW_B * (k0 + 4)));
  return r.u4;
}
