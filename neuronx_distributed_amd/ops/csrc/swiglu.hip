// Fused SwiGLU activation: out = silu(gate) * up, with [gate; up] packed in
// one tensor (the fused gate-up ColumnParallel GEMM output, reference
// modules/moe/experts.py:219-233 GLU path).  HBM-bound; vectorized.
//
// x (N, 2I) bf16 -> out (N, I) bf16;  bwd: dy (N, I) -> dx (N, 2I).

#include "transpose_tile.h"

extern "C" __global__ void __launch_bounds__(256)
swiglu_fwd_kernel(const short* __restrict__ x, short* __restrict__ out,
                  long N, int I) {
  // ONE int64 div/mod at entry, then carry-advance (row, i) each
  // iteration; v_rcp_f32 for the sigmoid (1-ulp fp32 — far below bf16
  // output rounding).
  int nvec = I >> 3;
  const long stride = (long)gridDim.x * blockDim.x;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long row = idx / nvec;
  int i = (int)(idx - row * nvec);
  const int di = (int)(stride % nvec);
  const long drow = stride / nvec;
  for (; idx < N * nvec; idx += stride) {
    const short* g = x + row * 2 * I + i * 8;
    const short* u = x + row * 2 * I + I + i * 8;
    s8v gv = *(const s8v*)g;
    s8v uv = *(const s8v*)u;
    s8v o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float gf = bits2f(gv[j]);
      float s = gf * __builtin_amdgcn_rcpf(
          1.f + __builtin_amdgcn_exp2f(-gf * 1.4426950408889634f));
      o[j] = f2bits(s * bits2f(uv[j]));
    }
    *(s8v*)(out + row * I + i * 8) = o;
    row += drow;
    i += di;
    if (i >= nvec) { i -= nvec; ++row; }
  }
}

// The backward of 8 elements, shared by both backward kernels so that their
// dx bits are the same instruction sequence.
__device__ __forceinline__ void swiglu_bwd8(s8v gv, s8v uv, s8v dv, s8v& dg,
                                            s8v& du) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float gf = bits2f(gv[j]);
    float df = bits2f(dv[j]);
    float sig = __builtin_amdgcn_rcpf(
        1.f + __builtin_amdgcn_exp2f(-gf * 1.4426950408889634f));
    float s = gf * sig;
    dg[j] = f2bits(df * bits2f(uv[j]) * (sig + s * (1.f - sig)));
    du[j] = f2bits(df * s);
  }
}

extern "C" __global__ void __launch_bounds__(256)
swiglu_bwd_kernel(const short* __restrict__ x, const short* __restrict__ dy,
                  short* __restrict__ dx, long N, int I) {
  // same div-free iteration + fast-rcp structure as the forward
  int nvec = I >> 3;
  const long stride = (long)gridDim.x * blockDim.x;
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long row = idx / nvec;
  int i = (int)(idx - row * nvec);
  const int di = (int)(stride % nvec);
  const long drow = stride / nvec;
  for (; idx < N * nvec; idx += stride) {
    const short* g = x + row * 2 * I + i * 8;
    const short* u = x + row * 2 * I + I + i * 8;
    const short* d = dy + row * I + i * 8;
    s8v gv = *(const s8v*)g;
    s8v uv = *(const s8v*)u;
    s8v dv = *(const s8v*)d;
    s8v dg, du;
    swiglu_bwd8(gv, uv, dv, dg, du);
    *(s8v*)(dx + row * 2 * I + i * 8) = dg;
    *(s8v*)(dx + row * 2 * I + I + i * 8) = du;
    row += drow;
    i += di;
    if (i >= nvec) { i -= nvec; ++row; }
  }
}

// Backward that also writes dxt (2I, N), the contiguous transpose of dx, for
// the K-contiguous gate_up weight gradient: one extra write of dx instead of
// a transpose pass that reads dx back.
//
// One 256-thread block owns 64 rows x 64 i (gate/up column pairs): the two
// 64x64 output tiles dx[:, i] and dx[:, I + i], which need the same g and dy
// loads.  Thread (ch = t&7, rp = t>>3) computes 8 columns of rows 2rp and
// 2rp+1 exactly as swiglu_bwd_kernel does, stores them to dx from registers
// (16 bytes per lane) and puts them into two LDS images of the transposed
// tiles (transpose_tile.h: the image, chunk swizzle and banking of
// transpose.hip, once per half; the second image starts 2048 dwords on, so
// it falls on the same banks).  After the barrier every thread stores two
// 16-byte chunks of dxt per image: rows [0, I) gate, [I, 2I) up.
//
// Edges: N and I are multiples of 8, so a chunk and a row pair are wholly
// inside or outside; outside lanes neither load nor store, and the dxt pass
// reads only LDS words that in-range lanes wrote.
extern "C" __global__ void __launch_bounds__(256)
swiglu_bwd_t_kernel(const short* __restrict__ x,
                    const short* __restrict__ dy, short* __restrict__ dx,
                    short* __restrict__ dxt, int N, int I, int tiles_i) {
  __shared__ __attribute__((aligned(16))) unsigned img[2 * TR_IMAGE_DWORDS];
  const int t = threadIdx.x;
  const int b = blockIdx.x;
  const int r0 = (b / tiles_i) * TR_TILE, i0 = (b % tiles_i) * TR_TILE;
  {
    const int ch = t & 7, rp = t >> 3;
    const int r = r0 + 2 * rp, i = i0 + 8 * ch;
    if (r < N && i < I) {
      const short* g = x + (long)r * 2 * I + i;
      const short* d = dy + (long)r * I + i;
      s8v g0 = *(const s8v*)g, u0 = *(const s8v*)(g + I);
      s8v g1 = *(const s8v*)(g + 2 * (long)I);
      s8v u1 = *(const s8v*)(g + 3 * (long)I);
      s8v d0 = *(const s8v*)d, d1 = *(const s8v*)(d + I);
      s8v dg0, du0, dg1, du1;
      swiglu_bwd8(g0, u0, d0, dg0, du0);
      swiglu_bwd8(g1, u1, d1, dg1, du1);
      short* o = dx + (long)r * 2 * I + i;
      *(s8v*)o = dg0;
      *(s8v*)(o + I) = du0;
      *(s8v*)(o + 2 * (long)I) = dg1;
      *(s8v*)(o + 3 * (long)I) = du1;
      tr_image_put(img, ch, rp, __builtin_bit_cast(u4v, dg0),
                   __builtin_bit_cast(u4v, dg1));
      tr_image_put(img + TR_IMAGE_DWORDS, ch, rp,
                   __builtin_bit_cast(u4v, du0),
                   __builtin_bit_cast(u4v, du1));
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int cl = it * 32 + (t >> 3), q = t & 7;
    const int i = i0 + cl, r = r0 + 8 * q;
    if (i < I && r < N) {
      short* o = dxt + (long)i * N + r;
      *(u4v*)o = tr_image_get(img, cl, q);
      *(u4v*)(o + (long)I * N) = tr_image_get(img + TR_IMAGE_DWORDS, cl, q);
    }
  }
}

extern "C" void swiglu_fwd(const void* x, void* out, long N, int I,
                           hipStream_t stream) {
  long work = N * (I >> 3);
  int blocks = (int)((work + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  swiglu_fwd_kernel<<<blocks, 256, 0, stream>>>((const short*)x, (short*)out,
                                                N, I);
}

extern "C" void swiglu_bwd(const void* x, const void* dy, void* dx, long N,
                           int I, hipStream_t stream) {
  long work = N * (I >> 3);
  int blocks = (int)((work + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  swiglu_bwd_kernel<<<blocks, 256, 0, stream>>>((const short*)x,
                                                (const short*)dy, (short*)dx,
                                                N, I);
}

// dx (N, 2I) as swiglu_bwd, plus dxt (2I, N) = dx^T.  Contract: N and I
// positive multiples of 8, 16-byte aligned pointers; returns nonzero and
// launches nothing otherwise.
extern "C" int swiglu_bwd_t(const void* x, const void* dy, void* dx,
                            void* dxt, long N, long I, hipStream_t stream) {
  if (N <= 0 || I <= 0 || (N & 7) || (I & 7) || N > 0x7fffffffL ||
      2 * I > 0x7fffffffL)
    return 1;
  if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)dxt) & 15)
    return 1;
  const long tiles_i = (I + TR_TILE - 1) / TR_TILE;
  const long blocks = ((N + TR_TILE - 1) / TR_TILE) * tiles_i;
  if (blocks > 0x7fffffffL) return 1;
  swiglu_bwd_t_kernel<<<(unsigned)blocks, 256, 0, stream>>>(
      (const short*)x, (const short*)dy, (short*)dx, (short*)dxt, (int)N,
      (int)I, (int)tiles_i);
  return 0;
}
