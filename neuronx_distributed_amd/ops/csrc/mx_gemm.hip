// Native MX (MXFP8 / MXFP4) linear on the gfx950 block-scaled MFMA.
//
//   mx_quantize_rows : bf16 (M,K) -> e4m3 payload (M,K) + e8m0 scales (M,K/32)
//   mx_gemm          : C(M,N) = A_mx(M,K) . W_mx(N,K)^T  (+ bias), bf16 | fp32
//
// Storage format (quantization/microscaling.py pack_mx): fp8 payload is one
// e4m3fn byte per element; fp4 payload is two e2m1 codes per byte, element
// 2i in the low nibble; scales are biased e8m0 bytes, one per 32 k.
//
// mx_gemm: 256 threads = 4 waves as 2(M) x 2(N), 128x128 output tile, K step
// 128.  A, W and their scale bytes are staged global -> registers -> LDS in
// two buffers: the loads of tile k+1 are issued before the MFMAs of tile k
// and written to the other buffer after them, one barrier per K step.  The
// fp4 tile is staged as stored (64-byte rows), never expanded.  Fragments are
// read k-contiguous with ds_read_b128 from the XOR-swizzled images of
// mx_mfma.h (fp4: one 16-byte MX block; fp8: two 16-byte half blocks).  W is the instruction's A operand and x
// its B operand, so a lane's four accumulators are four consecutive n of one
// m and the epilogue stores 8 (bf16) or 16 (fp32) contiguous bytes.
//
// Ragged tiles: rows past M (N) are loaded from the clamped last row and
// their results are never stored.  K % 128 == 0, N % 16 == 0, M >= 1.
//
// This 128x128 tile is the prefill configuration.  At M <= 32 three quarters
// of its x tile is padding and N/128 workgroups do not fill the machine:
// decode goes through mx_skinny.hip (M-skinny, split-K, the activation
// quantized inside the GEMM), which ops.mx_linear dispatches to.  The
// quantizer itself is shared with it through mx_quant.h.

#include "mx_mfma.h"
#include "mx_quant.h"

#define MXG_BM 128
#define MXG_BN 128
#define MXG_BK 128
#define MXG_A_B (MXG_BM * MXG_BK)             // 16384: fp8 x tile
#define MXG_W_B (MXG_BN * MXG_BK)             // 16384: fp8 W tile (fp4: half)
#define MXG_LDS_A 0
#define MXG_LDS_W MXG_A_B
#define MXG_LDS_SA (MXG_A_B + MXG_W_B)
#define MXG_LDS_SW (MXG_LDS_SA + MX_SIMG_B)
#define MXG_BUF_B (MXG_LDS_SW + MX_SIMG_B)    // 33792 B per buffer
#define MXG_LDS_TOTAL (2 * MXG_BUF_B)         // 67584 B

// ---------------------------------------------------------------------------
// mx_quantize_rows: one thread per 32-element block.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
mx_quantize_rows_kernel(const short* __restrict__ x, long row_stride,
                        uint8_t* __restrict__ q, uint8_t* __restrict__ s,
                        int M, int K) {
  const int kbpr = K / 32;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)M * kbpr) return;
  const long row = idx / kbpr;
  const int kb = (int)(idx - row * kbpr);

  const s8v* src = (const s8v*)(x + row * row_stride + 32 * kb);
  s8v v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = src[i];

  // the quantizer proper lives in mx_quant.h
  uint4v out[2];
  const int e = mxq_block32(v, out);
  uint4v* dst = (uint4v*)(q + row * K + 32 * kb);
  dst[0] = out[0];
  dst[1] = out[1];
  s[idx] = (uint8_t)(e + 127);
}

extern "C" int mx_quantize_rows(const void* x, long row_stride, void* q,
                                void* s, int M, int K, hipStream_t stream) {
  if (M < 1 || K < 32 || K % 32 != 0 || row_stride < K || row_stride % 8 != 0)
    return 1;
  const long nblk = (long)M * (K / 32);
  const long grid = (nblk + 255) / 256;
  if (grid > 0x7FFFFFFFL) return 1;
  mx_quantize_rows_kernel<<<(unsigned)grid, 256, 0, stream>>>(
      (const short*)x, row_stride, (uint8_t*)q, (uint8_t*)s, M, K);
  return 0;
}

// ---------------------------------------------------------------------------
// mx_gemm
// ---------------------------------------------------------------------------
template <int WFMT>
struct MxStage {
  static constexpr int WRB = (WFMT == MX_FMT_E2M1) ? 64 : 128;  // W row bytes
  static constexpr int WCH = WRB / 16;
  static constexpr int WLD = WCH / 2;  // 16-byte W loads per thread per tile
  uint4v a[4];
  uint4v w[WLD];
  unsigned sc;

  // rows are pre-clamped: every address is inside the operand
  __device__ __forceinline__ void load(const uint8_t* __restrict__ A,
                                       const uint8_t* __restrict__ W,
                                       const uint8_t* __restrict__ sA,
                                       const uint8_t* __restrict__ sW,
                                       int m0, int n0, int M, int N, int K,
                                       int kt, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      const int row = min(m0 + (c >> 3), M - 1);
      a[i] = *(const uint4v*)(A + (long)row * K + MXG_BK * kt + 16 * (c & 7));
    }
    const long w_rs = (WFMT == MX_FMT_E2M1) ? K / 2 : K;
#pragma unroll
    for (int i = 0; i < WLD; ++i) {
      const int c = tid + 256 * i;
      const int row = min(n0 + c / WCH, N - 1);
      w[i] = *(const uint4v*)(W + row * w_rs + WRB * kt + 16 * (c % WCH));
    }
    const int s_rs = K / 32;
    if (tid < 128) {
      const int row = min(m0 + tid, M - 1);
      sc = *(const unsigned*)(sA + (long)row * s_rs + 4 * kt);
    } else {
      const int row = min(n0 + tid - 128, N - 1);
      sc = *(const unsigned*)(sW + (long)row * s_rs + 4 * kt);
    }
  }

  __device__ __forceinline__ void store(char* buf, int tid) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      *(uint4v*)(buf + MXG_LDS_A + mx_off<128>(c >> 3, c & 7)) = a[i];
    }
#pragma unroll
    for (int i = 0; i < WLD; ++i) {
      const int c = tid + 256 * i;
      *(uint4v*)(buf + MXG_LDS_W + mx_off<WRB>(c / WCH, c % WCH)) = w[i];
    }
    char* simg = buf + (tid < 128 ? MXG_LDS_SA : MXG_LDS_SW);
    const int row = tid & 127;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      simg[mx_soff(row, kb)] = (char)(sc >> (8 * kb));
  }
};

// one m-fragment against the four n-fragments; op_sel = fragment index
#define MX_MMA_ROW(MI)                                                        \
  acc[MI][0] = mfma_mx<WFMT, MX_FMT_E4M3, 0, MI>(wf[0], xf[MI], acc[MI][0],   \
                                                 sw, sx);                     \
  acc[MI][1] = mfma_mx<WFMT, MX_FMT_E4M3, 1, MI>(wf[1], xf[MI], acc[MI][1],   \
                                                 sw, sx);                     \
  acc[MI][2] = mfma_mx<WFMT, MX_FMT_E4M3, 2, MI>(wf[2], xf[MI], acc[MI][2],   \
                                                 sw, sx);                     \
  acc[MI][3] = mfma_mx<WFMT, MX_FMT_E4M3, 3, MI>(wf[3], xf[MI], acc[MI][3],   \
                                                 sw, sx);

template <int WFMT, typename OutT>
__global__ void __launch_bounds__(256)
mx_gemm_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ sA,
               const uint8_t* __restrict__ W, const uint8_t* __restrict__ sW,
               const float* __restrict__ bias, OutT* __restrict__ C, int M,
               int N, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;  // wave's 64x64 sub-tile
  const int fr = lane & 15, fq = lane >> 4;
  const int m0 = blockIdx.y * MXG_BM, n0 = blockIdx.x * MXG_BN;
  const int KT = K / MXG_BK;

  f32x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  MxStage<WFMT> st;
  st.load(A, W, sA, sW, m0, n0, M, N, K, 0, tid);
  st.store(smem, tid);
  __syncthreads();

  for (int kt = 0; kt < KT; ++kt) {
    const char* buf = smem + (kt & 1) * MXG_BUF_B;
    const bool more = kt + 1 < KT;
    if (more) st.load(A, W, sA, sW, m0, n0, M, N, K, kt + 1, tid);

    i32x8 xf[4], wf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xf[i] = mx_frag_read<MX_FMT_E4M3>(buf + MXG_LDS_A,
                                        64 * wr + 16 * i + fr, fq);
      wf[i] = mx_frag_read<WFMT>(buf + MXG_LDS_W, 64 * wc + 16 * i + fr, fq);
    }
    const int sx = mx_scale_read(buf + MXG_LDS_SA, lane, 4 * wr);
    const int sw = mx_scale_read(buf + MXG_LDS_SW, lane, 4 * wc);

    MX_MMA_ROW(0)
    MX_MMA_ROW(1)
    MX_MMA_ROW(2)
    MX_MMA_ROW(3)

    // the other buffer was last read before the previous barrier
    if (more) st.store(smem + ((kt + 1) & 1) * MXG_BUF_B, tid);
    __syncthreads();
  }

  // D row = n (4*fq + r), D col = m (fr): four consecutive n per lane
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = m0 + 64 * wr + 16 * mi + fr;
    if (m >= M) continue;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + 64 * wc + 16 * ni + 4 * fq;
      if (n >= N) continue;  // N % 16 == 0: a fragment is all in or all out
      f32x4 v = acc[mi][ni];
      if (bias != nullptr) v += *(const f32x4*)(bias + n);
      mx_store4<OutT>(C + (long)m * N + n, v);
    }
  }
}

template <int WFMT, typename OutT>
static void mx_gemm_launch(const void* a, const void* sa, const void* w,
                           const void* sw, const void* bias, void* c, int M,
                           int N, int K, hipStream_t stream) {
  dim3 grid((N + MXG_BN - 1) / MXG_BN, (M + MXG_BM - 1) / MXG_BM);
  mx_gemm_kernel<WFMT, OutT><<<grid, 256, MXG_LDS_TOTAL, stream>>>(
      (const uint8_t*)a, (const uint8_t*)sa, (const uint8_t*)w,
      (const uint8_t*)sw, (const float*)bias, (OutT*)c, M, N, K);
}

// w_fmt: 0 = e4m3, 4 = e2m1 (the instruction's format codes); out_fp32: 0 =
// bf16, 1 = fp32; bias: fp32 (N) or null.  Returns nonzero WITHOUT launching
// when the shape or format is outside the contract.
extern "C" int mx_gemm(const void* a, const void* sa, const void* w,
                       const void* sw, const void* bias, void* c, int M, int N,
                       int K, int w_fmt, int out_fp32, hipStream_t stream) {
  if (M < 1 || N < 16 || N % 16 != 0 || K < MXG_BK || K % MXG_BK != 0)
    return 1;
  if ((M + MXG_BM - 1) / MXG_BM > 65535) return 1;
  if (w_fmt != MX_FMT_E4M3 && w_fmt != MX_FMT_E2M1) return 2;
  if (w_fmt == MX_FMT_E2M1) {
    if (out_fp32)
      mx_gemm_launch<MX_FMT_E2M1, float>(a, sa, w, sw, bias, c, M, N, K, stream);
    else
      mx_gemm_launch<MX_FMT_E2M1, bf16>(a, sa, w, sw, bias, c, M, N, K, stream);
  } else {
    if (out_fp32)
      mx_gemm_launch<MX_FMT_E4M3, float>(a, sa, w, sw, bias, c, M, N, K, stream);
    else
      mx_gemm_launch<MX_FMT_E4M3, bf16>(a, sa, w, sw, bias, c, M, N, K, stream);
  }
  return 0;
}
