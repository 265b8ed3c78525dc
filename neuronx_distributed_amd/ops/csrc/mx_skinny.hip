// Skinny (M <= 32) MX linear for decode, on the gfx950 block-scaled MFMA:
//
//   mx_skinny_gemm : y(M,N) = quant_mxfp8(x)(M,K) . W_mx(N,K)^T (+ bias)
//
// x is bf16 and is quantized to MXFP8 INSIDE the kernel with the pieces of
// mx_quant.h, i.e. to the very bytes mx_quantize_rows would store; W is the
// stored MX payload of mx_gemm.hip (e4m3 (N,K) or e2m1 (N,K/2), e8m0 scales
// (N,K/32)).  The work at these sizes is streaming W once, so:
//
// * No LDS on the operand path.  A workgroup owns NB = 16*NF consecutive n
//   rows (NF = 1 for M <= 16, 2 above) and a range of 128-deep K steps.  Each
//   lane loads its W fragment from global memory straight into the MFMA's
//   register layout of mx_mfma.h (lane (i, g): row i, fp4 16 bytes at byte
//   16*g of the row's 64-byte step, fp8 16 bytes at 16*g and at 64 + 16*g)
//   and its scale byte (row i, block g).  Every W and scale byte is read by
//   exactly one lane of one workgroup.
// * x fragments are built in the same layout: lane (i, g) reads row i's
//   k = 16*g.. and 64 + 16*g.. runs (16 bf16 each), which are HALVES of MX
//   blocks g>>1 and 2 + (g>>1); the block amax is completed with the lane
//   16 away, and the scale byte the instruction wants in lane (i, g) -- that
//   of block g -- is fetched from the lane that computed it.
// * K is split inside the workgroup first: wave w takes K steps w, w+4, ...
//   of the workgroup's range, and the four partial accumulators are summed
//   through LDS in wave order.  On top of that gridDim.y = KS workgroups
//   split K when N/NB alone does not fill the machine; then the fp32
//   partials go to workspace (KS, M, N) and mx_skinny_reduce sums them in
//   slice order, adds the bias and stores.  With KS == 1 the main kernel
//   stores the final output itself.  No atomics, no cross-workgroup hand-off
//   inside a kernel: results are bitwise reproducible.
// * The W loads of a group of K steps (32 registers per lane: 8 steps of fp4
//   or 4 of fp8 at NF = 1) are issued before the first is consumed, and the
//   next group's before the current one is computed.
//
// W stays the instruction's A operand, so a lane ends with four consecutive
// n of one m.  Rows past M (N) are loaded from the clamped last row and never
// stored.  Contract: 1 <= M <= 32, K % 128 == 0, N % 16 == 0, x rows dense
// with a 16-byte-multiple stride.

#include "mx_mfma.h"
#include "mx_quant.h"

#define MXS_BK 128
#define MXS_MAX_M 32

template <int WFMT>
__device__ __forceinline__ i32x8 mxs_load_w(const uint8_t* p) {
  union { i32x8 v; i32x4 h[2]; } r;
  r.h[0] = *(const i32x4*)p;
  if constexpr (WFMT == MX_FMT_E2M1)
    r.h[1] = i32x4{0, 0, 0, 0};
  else
    r.h[1] = *(const i32x4*)(p + 64);
  return r.v;
}

// W fragments and scale bytes of one K step (scale of fragment j in byte j)
template <int WFMT, int NF>
struct MxsW {
  i32x8 f[NF];
  int sc;
  __device__ __forceinline__ void load(const uint8_t* (&wr)[NF],
                                       const uint8_t* (&sr)[NF],
                                       int kt) {
    constexpr int STEP_B = (WFMT == MX_FMT_E2M1) ? 64 : 128;
    sc = 0;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      f[j] = mxs_load_w<WFMT>(wr[j] + (long)STEP_B * kt);
      sc |= (int)sr[j][4 * kt] << (8 * j);
    }
  }
};

// Quantize this lane's two 16-element runs of row `xr` at K step kt into the
// fp8 B-operand registers; returns the biased scale byte of block g.
__device__ __forceinline__ int mxs_quant_frag(const short* xr, int kt, int lane,
                                              i32x8& out) {
  const s8v* p = (const s8v*)(xr + MXS_BK * kt);
  const s8v a0 = p[0], a1 = p[1];  // k = 16g .. 16g+15      (block g>>1)
  const s8v b0 = p[8], b1 = p[9];  // k = 64+16g .. 64+16g+15 (block 2+(g>>1))
  int aba = mxq_amax_bits(a1, mxq_amax_bits(a0, 0));
  int abb = mxq_amax_bits(b1, mxq_amax_bits(b0, 0));
  // the other half of each block is in the lane 16 away (g ^ 1)
  aba = max(aba, __shfl_xor(aba, 16, 64));
  abb = max(abb, __shfl_xor(abb, 16, 64));
  const int ea = mxq_block_exp(aba), eb = mxq_block_exp(abb);
  const float ia = mxq_inv_scale(ea), ib = mxq_inv_scale(eb);
  unsigned w[8];
  mxq_cvt8(a0, ia, w[0], w[1]);
  mxq_cvt8(a1, ia, w[2], w[3]);
  mxq_cvt8(b0, ib, w[4], w[5]);
  mxq_cvt8(b1, ib, w[6], w[7]);
#pragma unroll
  for (int r = 0; r < 8; ++r) out[r] = (int)w[r];
  // lane group g holds blocks (g>>1, 2 + (g>>1)) and must present block g:
  // g = 0 own first, g = 1 first of g = 2, g = 2 second of g = 1, g = 3 own
  // second.
  const int g = lane >> 4;
  const int mine = (ea + 127) | ((eb + 127) << 8);
  const int src = lane + (g == 1 ? 16 : (g == 2 ? -16 : 0));
  const int got = __shfl(mine, src, 64);
  return (g < 2) ? (got & 0xFF) : ((got >> 8) & 0xFF);
}

template <int WFMT, int MF, int NF>
__device__ __forceinline__ void mxs_step(const short* (&xr)[MF], int kt,
                                         int lane, const MxsW<WFMT, NF>& w,
                                         f32x4 (&acc)[MF][NF]) {
  i32x8 xf[MF];
  int sx = 0;
#pragma unroll
  for (int f = 0; f < MF; ++f)
    sx |= mxs_quant_frag(xr[f], kt, lane, xf[f]) << (8 * f);
  // op_sel = fragment index on both sides
  acc[0][0] = mfma_mx<WFMT, MX_FMT_E4M3, 0, 0>(w.f[0], xf[0], acc[0][0],
                                               w.sc, sx);
  if constexpr (NF > 1)
    acc[0][1] = mfma_mx<WFMT, MX_FMT_E4M3, 1, 0>(w.f[1], xf[0], acc[0][1],
                                                 w.sc, sx);
  if constexpr (MF > 1) {
    acc[1][0] = mfma_mx<WFMT, MX_FMT_E4M3, 0, 1>(w.f[0], xf[1], acc[1][0],
                                                 w.sc, sx);
    if constexpr (NF > 1)
      acc[1][1] = mfma_mx<WFMT, MX_FMT_E4M3, 1, 1>(w.f[1], xf[1], acc[1][1],
                                                   w.sc, sx);
  }
}

// U consecutive K steps of this wave (kt, kt+4, ...): all W loads first
template <int WFMT, int MF, int NF, int U>
__device__ __forceinline__ void mxs_group(const short* (&xr)[MF],
                                          const uint8_t* (&wr)[NF],
                                          const uint8_t* (&sr)[NF],
                                          int kt, int lane,
                                          f32x4 (&acc)[MF][NF]) {
  MxsW<WFMT, NF> w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) w[u].load(wr, sr, kt + 4 * u);
#pragma unroll
  for (int u = 0; u < U; ++u)
    mxs_step<WFMT, MF, NF>(xr, kt + 4 * u, lane, w[u], acc);
}

// grid (ceil(N / (16*NF)), KS).  part != null: fp32 partials (KS, M, N), no
// bias; else the final output.
template <int WFMT, int MF, int NF, typename OutT>
__global__ void __launch_bounds__(256)
mx_skinny_kernel(const short* __restrict__ x, long row_stride,
                 const uint8_t* __restrict__ W, const uint8_t* __restrict__ sW,
                 const float* __restrict__ bias, OutT* __restrict__ out,
                 float* __restrict__ part, int M, int N, int K) {
  constexpr int NFR = MF * NF;
  // K steps per group: 32 W registers per lane, twice that in flight
  constexpr int U = ((WFMT == MX_FMT_E2M1) ? 8 : 4) / NF;
  __shared__ f32x4 red[4][NFR][64];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * (16 * NF);
  const int KT = K / MXS_BK;
  const int KS = gridDim.y, ks = blockIdx.y;
  const int kbeg = (int)((long)ks * KT / KS);
  const int kend = (int)((long)(ks + 1) * KT / KS);

  // rows are clamped: every address is inside the operand
  const short* xr[MF];
#pragma unroll
  for (int f = 0; f < MF; ++f)
    xr[f] = x + (long)min(16 * f + i, M - 1) * row_stride + 16 * g;
  const long w_rs = (WFMT == MX_FMT_E2M1) ? K / 2 : K;
  const uint8_t* wr[NF];
  const uint8_t* sr[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const long row = min(n0 + 16 * j + i, N - 1);
    wr[j] = W + row * w_rs + 16 * g;
    sr[j] = sW + row * (K / 32) + g;
  }

  f32x4 acc[MF][NF];
#pragma unroll
  for (int f = 0; f < MF; ++f)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[f][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int kt = kbeg + wid;
  if (kt + 4 * (U - 1) < kend) {
    // full groups, the next one's W loads in flight over this one's math
    MxsW<WFMT, NF> cur[U], nxt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u].load(wr, sr, kt + 4 * u);
    for (;;) {
      const bool more = kt + 4 * U + 4 * (U - 1) < kend;
      if (more) {
#pragma unroll
        for (int u = 0; u < U; ++u) nxt[u].load(wr, sr, kt + 4 * U + 4 * u);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        mxs_step<WFMT, MF, NF>(xr, kt + 4 * u, lane, cur[u], acc);
      kt += 4 * U;
      if (!more) break;
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
  }
  if constexpr (U >= 8) {
    if (kt + 12 < kend) {
      mxs_group<WFMT, MF, NF, 4>(xr, wr, sr, kt, lane, acc);
      kt += 16;
    }
  }
  if constexpr (U >= 4) {
    if (kt + 4 < kend) {
      mxs_group<WFMT, MF, NF, 2>(xr, wr, sr, kt, lane, acc);
      kt += 8;
    }
  }
  for (; kt < kend; kt += 4)
    mxs_group<WFMT, MF, NF, 1>(xr, wr, sr, kt, lane, acc);

  // in-workgroup K reduction: fragment f of every wave is summed by wave f,
  // in wave order
#pragma unroll
  for (int f = 0; f < MF; ++f)
#pragma unroll
    for (int j = 0; j < NF; ++j) red[wid][f * NF + j][lane] = acc[f][j];
  __syncthreads();
  if (wid >= NFR) return;
  f32x4 v = red[0][wid][lane];
  v += red[1][wid][lane];
  v += red[2][wid][lane];
  v += red[3][wid][lane];

  // D row = n (4*g + r), D col = m (i): four consecutive n per lane
  const int m = 16 * (wid / NF) + i;
  const int n = n0 + 16 * (wid % NF) + 4 * g;
  if (m >= M || n >= N) return;  // N % 16 == 0: a fragment is all in or out
  if (part != nullptr) {
    *(f32x4*)(part + ((long)ks * M + m) * N + n) = v;
  } else {
    if (bias != nullptr) v += *(const f32x4*)(bias + n);
    mx_store4<OutT>(out + (long)m * N + n, v);
  }
}

// out(M,N) = sum over slices, in slice order, of part(KS,M,N) (+ bias)
template <typename OutT>
__global__ void __launch_bounds__(256)
mx_skinny_reduce(const float* __restrict__ part, const float* __restrict__ bias,
                 OutT* __restrict__ out, int M, int N, int KS) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // one per 4 n
  const long total = (long)M * N / 4;
  if (idx >= total) return;
  const long slab = (long)M * N;
  const float* p = part + 4 * idx;
  f32x4 v = *(const f32x4*)p;
  for (int s = 1; s < KS; ++s) v += *(const f32x4*)(p + s * slab);
  if (bias != nullptr) v += *(const f32x4*)(bias + (4 * idx) % N);
  mx_store4<OutT>(out + 4 * idx, v);
}

template <int WFMT, int MF, int NF>
static void mxs_launch(const void* x, long row_stride, const void* w,
                       const void* sw, const void* bias, void* out, void* ws,
                       int M, int N, int K, int out_fp32, int KS,
                       hipStream_t stream) {
  dim3 grid((N + 16 * NF - 1) / (16 * NF), KS);
  float* part = KS > 1 ? (float*)ws : nullptr;
  if (out_fp32 || KS > 1)
    mx_skinny_kernel<WFMT, MF, NF, float><<<grid, 256, 0, stream>>>(
        (const short*)x, row_stride, (const uint8_t*)w, (const uint8_t*)sw,
        (const float*)bias, (float*)out, part, M, N, K);
  else
    mx_skinny_kernel<WFMT, MF, NF, bf16><<<grid, 256, 0, stream>>>(
        (const short*)x, row_stride, (const uint8_t*)w, (const uint8_t*)sw,
        (const float*)bias, (bf16*)out, part, M, N, K);
  if (KS > 1) {
    const unsigned rgrid = (unsigned)(((long)M * N / 4 + 255) / 256);
    if (out_fp32)
      mx_skinny_reduce<float><<<rgrid, 256, 0, stream>>>(
          part, (const float*)bias, (float*)out, M, N, KS);
    else
      mx_skinny_reduce<bf16><<<rgrid, 256, 0, stream>>>(
          part, (const float*)bias, (bf16*)out, M, N, KS);
  }
}

// x: bf16 (M, K) rows `row_stride` elements apart; w / sw / bias / w_fmt /
// out_fp32 as in mx_gemm.  k_splits >= 1 is clamped to K / 128; workspace
// holds (clamped k_splits, M, N) fp32 and may be null when that is 1.
// Returns nonzero WITHOUT launching outside the contract.
extern "C" int mx_skinny_gemm(const void* x, long row_stride, const void* w,
                              const void* sw, const void* bias, void* out,
                              void* workspace, int M, int N, int K, int w_fmt,
                              int out_fp32, int k_splits, hipStream_t stream) {
  if (M < 1 || M > MXS_MAX_M || N < 16 || N % 16 != 0 || K < MXS_BK ||
      K % MXS_BK != 0)
    return 1;
  if (row_stride < K || row_stride % 8 != 0) return 1;
  if (w_fmt != MX_FMT_E4M3 && w_fmt != MX_FMT_E2M1) return 2;
  if (k_splits < 1) return 3;
  const int KS = k_splits < K / MXS_BK ? k_splits : K / MXS_BK;
  if (KS > 65535) return 3;
  if (KS > 1 && workspace == nullptr) return 4;
  if (w_fmt == MX_FMT_E2M1) {
    if (M <= 16)
      mxs_launch<MX_FMT_E2M1, 1, 1>(x, row_stride, w, sw, bias, out, workspace,
                                    M, N, K, out_fp32, KS, stream);
    else
      mxs_launch<MX_FMT_E2M1, 2, 2>(x, row_stride, w, sw, bias, out, workspace,
                                    M, N, K, out_fp32, KS, stream);
  } else {
    if (M <= 16)
      mxs_launch<MX_FMT_E4M3, 1, 1>(x, row_stride, w, sw, bias, out, workspace,
                                    M, N, K, out_fp32, KS, stream);
    else
      mxs_launch<MX_FMT_E4M3, 2, 2>(x, row_stride, w, sw, bias, out, workspace,
                                    M, N, K, out_fp32, KS, stream);
  }
  return 0;
}
