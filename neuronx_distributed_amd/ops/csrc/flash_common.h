// Mechanisms shared by the three MFMA attention kernels (flash_fwd_kernel,
// fa_bwd_dkdv_kernel, fa_bwd_dq_kernel): tile staging into the dual-use LDS
// image of mfma.h, the accumulator -> fragment repack, the per-element mask
// predicate and the dense stride block.  A few call sites still write one
// of these out by hand because the helper changed that kernel's generated
// code; each says so where it does.
#pragma once

#include "common.h"
#include "mfma.h"

#define FA_D 128
#define LOG2E 1.4426950408889634f

// Stage a 64x128 bf16 tile ONCE, in the dual-use image of mfma.h (256-byte
// rows, chunk XOR of img_off): the same copy feeds the ds_read_b128 row
// reads (A fragments of the score mfmas) and the ds_read_b64_tr_b16
// transposed reads (PV / dV / dK / dQ mfmas).  Thread t owns NR consecutive
// rows at 16-byte chunk t&15 (NR = 64*16 / blockDim.x), i.e. NR coalesced
// b128 global loads and NR ds_write_b128.  Rows past the end of the
// sequence are CLAMPED, never skipped: every image row always holds data,
// so the transposed reads run with all lanes active (pad, don't mask).
// The load and the write are separate calls so that a kernel can issue the
// next tile's loads early and write them to LDS late.
#define TILE64_B (64 * IMG_ROW_B)   // 16384 B

template <int NR>
struct StageRegs { uint4v v[NR]; };

template <int NR>
__device__ __forceinline__ StageRegs<NR> load_tile64(
    const short* __restrict__ src, long src_row0, long src_stride,
    int rows_valid) {
  const int rp = threadIdx.x >> 4;
  const int c16 = threadIdx.x & 15;
  const int last = rows_valid > 0 ? rows_valid - 1 : 0;
  StageRegs<NR> r;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    int row = NR * rp + i;
    int rr = row < rows_valid ? row : last;
    r.v[i] = *(const uint4v*)(src + (src_row0 + rr) * src_stride + c16 * 8);
  }
  return r;
}

template <int NR>
__device__ __forceinline__ void write_tile64(StageRegs<NR> r, char* img) {
  const int rp = threadIdx.x >> 4;
  const int c16 = threadIdx.x & 15;
#pragma unroll
  for (int i = 0; i < NR; ++i)
    *(uint4v*)(img + img_off(NR * rp + i, c16)) = r.v[i];
}

// Repack accumulator elements a[r0 .. r0+7] (r0 = 0 or 8: 16 consecutive
// tile rows, 8 per lane half) into the bf16 fragment whose k-dim is that
// row index; the lane dim is already in place.  4 packs + 2
// v_permlane32_swap (T12/T21), no LDS round-trip.  `a` is an f32x16 or a
// float[16].
template <typename Acc>
__device__ __forceinline__ frag_u acc8_to_frag(const Acc& a, int r0) {
  uint b0 = pack_bf16x2(a[r0 + 0], a[r0 + 1]);
  uint b1 = pack_bf16x2(a[r0 + 2], a[r0 + 3]);
  uint b2 = pack_bf16x2(a[r0 + 4], a[r0 + 5]);
  uint b3 = pack_bf16x2(a[r0 + 6], a[r0 + 7]);
  {
    auto r01 = __builtin_amdgcn_permlane32_swap(b0, b2, false, false);
    b0 = r01[0]; b2 = r01[1];
  }
  {
    auto r23 = __builtin_amdgcn_permlane32_swap(b1, b3, false, false);
    b1 = r23[0]; b3 = r23[1];
  }
  frag_u f;
  f.u[0] = b0; f.u[1] = b1; f.u[2] = b2; f.u[3] = b3;
  return f;
}

// Is score element (kv row kg, q row qg) masked out: above the causal
// diagonal, past the end of the sequence, or below the sliding window
// (q attends kv rows [q - window + 1, q]).  Bitwise | and &: plain compares
// + one select per element, no per-element branch.  CHECK_Q adds the q
// bound, which the backward needs because its clamped q rows carry real
// lse/delta; the forward simply never stores them.
template <bool CHECK_Q>
__device__ __forceinline__ bool fa_masked(int kg, int qg, int S, int causal,
                                          int window) {
  bool m = ((causal != 0) & (kg > qg)) | (kg >= S);
  if (CHECK_Q) m = m | (qg >= S);
  return m | ((window > 0) & (kg <= qg - window));
}

// Dense (B, H, S, 128) element strides (bs, hs, ss) for q, k, v, out in
// st[0..11]: the head of the stride block of both *_strided entry points.
static inline void fa_dense_strides(long* st, int Hq, int Hkv, int S) {
  const long qd[3] = {(long)Hq * S * FA_D, (long)S * FA_D, FA_D};
  const long kd[3] = {(long)Hkv * S * FA_D, (long)S * FA_D, FA_D};
  for (int i = 0; i < 3; ++i) {
    st[0 + i] = qd[i];            // q
    st[3 + i] = kd[i];            // k
    st[6 + i] = kd[i];            // v
    st[9 + i] = qd[i];            // out
  }
}
