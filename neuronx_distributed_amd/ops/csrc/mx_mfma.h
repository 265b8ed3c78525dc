// Block-scaled (MX) MFMA fragment helpers for
// v_mfma_scale_f32_16x16x128_f8f6f4 on gfx950.
//
// D(16x16) += A(16x128) * B(128x16), A and B in fp8 e4m3 (FMT 0) or fp4 e2m1
// (FMT 4), each 32-long k-block of a row/column scaled by 2^(e8m0 - 127).
//
// Layout contracts (measured on MI355X with one-hot data and one-hot scales,
// and pinned with exact integer data by
// tests/test_mx_gemm_gpu.py::test_exact_maps).  g = l>>4 is the lane group,
// i = l&15 the row of A / column of B; k is the index along K (0..127):
//   fp8 operand (8 registers, 32 bytes): the lane holds TWO 16-element runs,
//       registers 0..3: k = 16*g + j,       j = 0..15
//       registers 4..7: k = 64 + 16*g + j,  j = 0..15
//     element j of a run in byte j&3 of register j>>2 (memory order).  So a
//     lane's 32 elements are halves of MX blocks g>>1 and 2 + (g>>1), NOT
//     one block: an fp8 fragment is two 16-byte pieces of a k-contiguous row.
//   fp4 operand (registers 0..3, 16 bytes; registers 4..7 are ignored):
//       k = 32*g + j, j = 0..31, exactly one MX block; element j in nibble
//       j&1 (LOW nibble first) of byte j>>1 -- the stored MX payload order,
//       so a k-contiguous row loads with no reordering.
//   A is [i][k], B is [k][i]; both operands follow the same k map, and the
//   two formats mix freely (fp4 A x fp8 B here).
//   Scales: one 32-bit register per operand.  The byte selected by op_sel
//     (0..3) in lane l is the biased e8m0 scale of row/column i, MX block
//     kb = g (k = 32*g .. 32*g+31), whichever lanes hold that block's data.
//     The other three bytes are free, so one register carries the scales of
//     four different fragments and op_sel picks per instruction.
//   C/D accumulator (4 f32/lane): element r holds
//       row = 4*g + r,  col = i
//     (the shape's usual map; it does not depend on the operand formats).
#pragma once

#include "common.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int uint4v __attribute__((ext_vector_type(4)));

#define MX_FMT_E4M3 0
#define MX_FMT_E2M1 4

// FA/FB: operand formats (cbsz/blgp); SA/SB: scale byte selects (op_sel).
template <int FA, int FB, int SA, int SB>
__device__ __forceinline__ f32x4 mfma_mx(i32x8 a, i32x8 b, f32x4 c,
                                         int scale_a, int scale_b) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, b, c, FA, FB, SA, scale_a, SB, scale_b);
}

// Four consecutive n of one accumulator: 16 (fp32) or 8 (bf16) bytes.
template <typename OutT>
__device__ __forceinline__ void mx_store4(OutT* p, f32x4 v);
template <>
__device__ __forceinline__ void mx_store4<float>(float* p, f32x4 v) {
  *(f32x4*)p = v;
}
template <>
__device__ __forceinline__ void mx_store4<bf16>(bf16* p, f32x4 v) {
  uint2 r;
  r.x = ((unsigned)(unsigned short)f2bits(v[0])) |
        ((unsigned)(unsigned short)f2bits(v[1]) << 16);
  r.y = ((unsigned)(unsigned short)f2bits(v[2])) |
        ((unsigned)(unsigned short)f2bits(v[3]) << 16);
  *(uint2*)p = r;
}

// ---------------------------------------------------------------------------
// LDS image of a [rows][RB bytes] k-contiguous tile (RB = 128 for an fp8
// K=128 tile, 64 for the fp4 one).  The 16 lanes that fetch the same
// k-offset of 16 consecutive rows would all land on the same 16-byte slot of
// the 256-byte bank row; XORing the chunk index with the row's position
// above the bank row spreads them over all 16 slots (mfma.h::img_off is the
// same idea for 256-byte rows).  Stores and reads both go through mx_off().
// ---------------------------------------------------------------------------
template <int RB>
__device__ __forceinline__ int mx_off(int row, int ch) {
  constexpr int CH = RB / 16;          // chunks per row
  constexpr int RPB = 256 / RB;        // rows per bank row
  return RB * row + 16 * (ch ^ ((row / RPB) & (CH - 1)));
}

// The fragment of lane group q (0..3) for row `row` of a K=128 tile.
template <int FMT>
__device__ __forceinline__ i32x8 mx_frag_read(const char* img, int row,
                                              int q) {
  union { i32x8 v; i32x4 h[2]; } r;
  if constexpr (FMT == MX_FMT_E2M1) {
    r.h[0] = *(const i32x4*)(img + mx_off<64>(row, q));
    r.h[1] = i32x4{0, 0, 0, 0};
  } else {
    r.h[0] = *(const i32x4*)(img + mx_off<128>(row, q));
    r.h[1] = *(const i32x4*)(img + mx_off<128>(row, 4 + q));
  }
  return r.v;
}

// Scale image of a 128-row tile: byte [kb][row & 15][row >> 4], so the lane
// that owns (row & 15, kb) reads the scales of its row in four consecutive
// 16-row fragments with one aligned 4-byte load (grp = first fragment, a
// multiple of 4) and selects among them with op_sel.
#define MX_SIMG_B 512
__device__ __forceinline__ int mx_soff(int row, int kb) {
  return 128 * kb + 8 * (row & 15) + (row >> 4);
}
__device__ __forceinline__ int mx_scale_read(const char* simg, int lane,
                                             int grp) {
  return *(const int*)(simg + 128 * (lane >> 4) + 8 * (lane & 15) + grp);
}
