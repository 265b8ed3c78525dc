// Batched bf16 2-D transpose: src (R, C) with a row stride -> dst (C, R)
// contiguous.  A pure permutation, HBM-bound: every element is read once and
// written once, 16 bytes per lane on both sides.
//
// One 256-thread block moves one 64x64 tile through an 8 KiB LDS image of
// the TRANSPOSED tile (64 rows c of 32 dwords; dword d of row c holds
// src[2d][c] | src[2d+1][c] << 16).
//
//  load   thread t: chunk ch = t&7 (8 columns), row pair rp = t>>3.  Two
//         16-byte global loads (rows 2rp, 2rp+1), packed in registers into 8
//         dwords, one per column, stored with 8 ds_write_b32.
//  store  thread t, pass it: tile row cl = 32*it + (t>>3), chunk q = t&7.
//         One ds_read_b128 (rows 8q..8q+7 of column cl) -> one 16-byte store.
//
// Banking (profiles/KERNEL_NOTES.md rule: ds_write_b32 bank = dword mod 32
// over 32-lane halves; ds_read_b128 bank = dword mod 64 over the four
// 16-lane groups).  The rows are exactly 32 dwords, so unswizzled every
// write of a half-wave (8 columns x 4 row pairs) would land on 4 banks.
// 16-byte chunk `k` of row c is therefore kept at chunk k ^ ((c>>3)&7):
//  * write: a half-wave has ch = 0..7 and rp = 4B..4B+3, bank =
//    ((B ^ ch) << 2) | (rp & 3): 32 distinct banks.
//  * read: a wave reads 8 consecutive rows (same c>>3, so the same XOR) and
//    all 8 chunks of each, i.e. 1 KiB contiguous up to a chunk permutation
//    common to the 8 rows; each 16-lane group covers all 64 banks once.
//
// Edges: R, C and the source row stride are multiples of 8 (16-byte rows),
// so a 16-byte chunk and a row pair are wholly inside or wholly outside the
// matrix; outside lanes neither load nor store, and no LDS word that was
// not written is ever stored.

#include "transpose_tile.h"

__device__ __forceinline__ void transpose_tile(
    const short* __restrict__ src, short* __restrict__ dst, long src_stride,
    int R, int C, int tr, int tc, unsigned* tile) {
  const int t = threadIdx.x;
  const int ch = t & 7, rp = t >> 3;
  const int r0 = tr * TR_TILE, c0 = tc * TR_TILE;
  {
    const int r = r0 + 2 * rp, c = c0 + 8 * ch;
    if (r < R && c < C) {
      const short* p = src + (long)r * src_stride + c;
      u4v a = *(const u4v*)p;
      u4v b = *(const u4v*)(p + src_stride);
      tr_image_put(tile, ch, rp, a, b);
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int cl = it * 32 + (t >> 3), q = t & 7;
    const int c = c0 + cl, r = r0 + 8 * q;
    if (c < C && r < R) {
      *(u4v*)(dst + (long)c * R + r) = tr_image_get(tile, cl, q);
    }
  }
}

extern "C" __global__ void __launch_bounds__(256)
transpose_bf16_kernel(const short* __restrict__ src, short* __restrict__ dst,
                      long src_stride, int R, int C, int tiles_c) {
  __shared__ __attribute__((aligned(16))) unsigned tile[TR_IMAGE_DWORDS];
  const int b = blockIdx.x;
  transpose_tile(src, dst, src_stride, R, C, b / tiles_c, b % tiles_c, tile);
}

// One launch over many matrices.  desc: n rows of 6 int64
// {src, dst, src_stride, R, C, first tile}, first tile ascending from 0.
#define TR_DESC 6

extern "C" __global__ void __launch_bounds__(256)
transpose_bf16_batched_kernel(const long* __restrict__ desc, int n) {
  __shared__ __attribute__((aligned(16))) unsigned tile[TR_IMAGE_DWORDS];
  const int b = blockIdx.x;
  // last matrix whose first tile is <= b (block-uniform)
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (desc[(long)mid * TR_DESC + 5] <= b) lo = mid; else hi = mid - 1;
  }
  const long* d = desc + (long)lo * TR_DESC;
  const int R = (int)d[3], C = (int)d[4];
  const int tiles_c = (C + TR_TILE - 1) / TR_TILE;
  const int local = b - (int)d[5];
  transpose_tile((const short*)d[0], (short*)d[1], d[2], R, C,
                 local / tiles_c, local % tiles_c, tile);
}

// One launch over up to four matrices whose descriptors travel BY VALUE in
// the kernel arguments: no device table, so no host-to-device copy per
// call.  first[i] is the first tile of matrix i (first[0] == 0, ascending;
// INT_MAX for the unused slots), so a block finds its matrix with at most
// three compares.
#define TR_MULTI_MAX 4

struct TrMat {
  const short* src;
  short* dst;
  long src_stride;
  int R, C;
};

struct TrMulti {
  TrMat m[TR_MULTI_MAX];
  int first[TR_MULTI_MAX];
};

extern "C" __global__ void __launch_bounds__(256)
transpose_bf16_multi_kernel(const TrMulti p) {
  __shared__ __attribute__((aligned(16))) unsigned tile[TR_IMAGE_DWORDS];
  const int b = blockIdx.x;
  const int i = (b >= p.first[1]) + (b >= p.first[2]) + (b >= p.first[3]);
  const TrMat& m = p.m[i];
  const int tiles_c = (m.C + TR_TILE - 1) / TR_TILE;
  const int local = b - p.first[i];
  transpose_tile(m.src, m.dst, m.src_stride, m.R, m.C, local / tiles_c,
                 local % tiles_c, tile);
}

static inline long transpose_tiles(long R, long C) {
  return ((R + TR_TILE - 1) / TR_TILE) * ((C + TR_TILE - 1) / TR_TILE);
}

// Tiles of an (R, C) matrix, or -1 when the shape is outside the contract.
extern "C" long transpose_bf16_tiles(long R, long C, long src_stride) {
  if (R <= 0 || C <= 0 || (R & 7) || (C & 7) || (src_stride & 7) ||
      src_stride < C || R > 0x7fffffffL || C > 0x7fffffffL)
    return -1;
  long tiles = transpose_tiles(R, C);
  return tiles > 0x7fffffffL ? -1 : tiles;
}

extern "C" int transpose_bf16(const void* src, void* dst, long src_stride,
                              long R, long C, hipStream_t stream) {
  long tiles = transpose_bf16_tiles(R, C, src_stride);
  if (tiles < 0 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return 1;
  transpose_bf16_kernel<<<(unsigned)tiles, 256, 0, stream>>>(
      (const short*)src, (short*)dst, src_stride, (int)R, (int)C,
      (int)((C + TR_TILE - 1) / TR_TILE));
  return 0;
}

// n in [1, 4] matrices given as host arrays; every matrix is checked against
// the contract before anything is launched.
extern "C" int transpose_bf16_multi(const void* const* srcs,
                                    void* const* dsts,
                                    const long* src_strides, const long* Rs,
                                    const long* Cs, int n,
                                    hipStream_t stream) {
  if (n < 1 || n > TR_MULTI_MAX) return 1;
  TrMulti p;
  long first = 0;
  for (int i = 0; i < TR_MULTI_MAX; ++i) {
    if (i >= n) {
      p.m[i] = TrMat{nullptr, nullptr, 0, 0, 0};
      p.first[i] = 0x7fffffff;
      continue;
    }
    long tiles = transpose_bf16_tiles(Rs[i], Cs[i], src_strides[i]);
    if (tiles < 0 || ((uintptr_t)srcs[i] & 15) || ((uintptr_t)dsts[i] & 15))
      return 1;
    p.m[i] = TrMat{(const short*)srcs[i], (short*)dsts[i], src_strides[i],
                   (int)Rs[i], (int)Cs[i]};
    p.first[i] = (int)first;
    first += tiles;
    if (first >= 0x7fffffffL) return 1;
  }
  transpose_bf16_multi_kernel<<<(unsigned)first, 256, 0, stream>>>(p);
  return 0;
}

// desc is DEVICE memory, validated by the caller (ops.transpose_batched
// builds it from tensors with transpose_bf16_tiles); total_tiles is the sum
// of the matrices' tile counts.
extern "C" int transpose_bf16_batched(const void* desc, int n,
                                      long total_tiles, hipStream_t stream) {
  if (n <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffffL) return 1;
  transpose_bf16_batched_kernel<<<(unsigned)total_tiles, 256, 0, stream>>>(
      (const long*)desc, n);
  return 0;
}
