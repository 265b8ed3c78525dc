// FlashAttention forward for CDNA4 (gfx950) — hand-written MFMA kernel.
//
// Replaces the reference's NKI flash kernels K1 (SURVEY.md §2.3,
// reference kernels/flash_attn.py:18,51-63).  MI355X-first design per
// cdna_hip_programming.md §B:
//   * 8 waves/WG, each wave owns 32 q rows (WG = 256 q rows); KV tiles of
//     64 rows in two staging buffers, one barrier per tile.  K and V are
//     each stored ONCE per tile in the dual-use LDS image of mfma.h
//     (256-byte rows, 16-byte chunks XORed by img_off): K is read row-wise
//     (ds_read_b128, A operand of QK^T), V transposed
//     (ds_read_b64_tr_b16, A operand of PV).
//   * swapped QK^T — mfma(A=K, B=Q^T) — so each lane's softmax stats are
//     for ONE q row (l&31): row max / rescale / denom are lane-local
//     (+ one shfl_xor with the partner half-wave).
//   * P is repacked to bf16 PV B-fragments with pack_bf16x2 +
//     v_permlane32_swap (T12/T21 primitive).
//   * O is accumulated TRANSPOSED (O^T[d][q], q = lane) so the online
//     rescale is a per-lane scalar multiply; the epilogue transposes it
//     back through LDS and stores whole 256-byte rows.
//   * GQA: kv head = q head / (Hq/Hkv); causal masking per element on
//     diagonal tiles, whole-tile skip below the diagonal.
//
// Layouts: q,k,v,out (B, H, S, D)-indexed bf16 with any (batch, head, seq)
// strides and a dense d, D = 128; lse (B,Hq,S) f32 contiguous
// (natural-log row logsumexp, saved for backward).

#include "flash_common.h"

#define FA_QW 32       // q rows per wave
#define FA_WAVES 8
#define FA_QBLK (FA_QW * FA_WAVES)  // 256 q rows per workgroup
#define FA_KV 64       // kv tile
#define NEG_INF (-1e30f)

// LDS: two staging buffers, each one K image + one V image of a 64-row tile
// (mfma.h dual-use image, 256-byte rows).  After the kv loop the same
// memory holds the 8 per-wave 32x128 O tiles of the epilogue.
#define FA_BUF_B (2 * TILE64_B)         // K image, then V image
#define FA_LDS_V TILE64_B
#define FA_LDS_TOTAL (2 * FA_BUF_B)     // 65,536 B

// The second launch-bound is HIP's minimum waves per SIMD, not blocks per
// CU: 2 waves/SIMD is exactly one 8-wave workgroup per CU.  The 64 KB of
// LDS would admit a second workgroup; the ~250 VGPRs per lane do not.
extern "C" __global__ void __launch_bounds__(512, 2)
flash_fwd_kernel(const short* __restrict__ qp, const short* __restrict__ kp,
                 const short* __restrict__ vp, short* __restrict__ op,
                 float* __restrict__ lsep, int B, int Hq, int Hkv, int S,
                 float scale, int causal, int window,
                 long q_bs, long q_hs, long q_ss,
                 long k_bs, long k_hs, long k_ss,
                 long v_bs, long v_hs, long v_ss,
                 long o_bs, long o_hs, long o_ss) {
  // (*_bs, *_hs, *_ss) = element strides of (batch, head, seq); the last
  // dim (d) is always dense.  BHSD contiguous: (H*S*128, S*128, 128).
  // BSHD transpose views (no-copy model layout): (S*H*128, 128, H*128).
  // window > 0: Mistral-style sliding window — q row i attends kv rows
  // [i - window + 1, i] (causal implied); whole tiles outside the band
  // are skipped, boundary tiles masked per element.
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63;
  // readfirstlane: provably wave-uniform -> scalar branches for the
  // per-wave activity guards instead of exec-mask divergence (T20)
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 31;       // q column owned by this lane
  const int hi = lane >> 5;

  // Dispatch mapping (causal LPT): heads on x, q-blocks on y REVERSED so
  // the largest-causal-work blocks launch first.  With x = q-block the
  // hardware pairs CU c with the SAME q-block index every occupancy round
  // (512 WGs / 256 CUs at 1 WG/CU) -> worst CUs do ~1.9x the mean causal
  // work while others idle; biggest-first lets early finishers absorb the
  // small diagonal blocks (greedy LPT, near-ideal pairing).
  const int qblk = (int)(gridDim.y - 1 - blockIdx.y);
  const int h = blockIdx.x;
  const int b = blockIdx.z;
  const int hkv = h / (Hq / Hkv);

  const long q_base = (long)b * q_bs + (long)h * q_hs;
  const long kv_base_k = (long)b * k_bs + (long)hkv * k_hs;
  const long kv_base_v = (long)b * v_bs + (long)hkv * v_hs;

  const int q0 = qblk * FA_QBLK;
  const int qw0 = q0 + wid * FA_QW;      // this wave's first q row
  const int my_q = qw0 + col;            // this lane's q row
  const int q_row_ld = my_q < S ? my_q : S - 1;

  // ---- Q fragments: 8 chunks of (16 d), each lane 8 bf16 --------------
  frag_u qf[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const short* src = qp + q_base + (long)q_row_ld * q_ss + c * 16 + hi * 8;
    qf[c].u4 = *(const uint4v*)src;
  }

  // ---- accumulators ----------------------------------------------------
  f32x16 ot[4] = {};          // O^T: d-block nb, rows d_local, col q
  float m_run = NEG_INF;      // running max (exp2 domain)
  float l_run = 0.f;

  const int kv_end = causal ? min(S, q0 + FA_QBLK) : S;
  const int ntiles = (kv_end + FA_KV - 1) / FA_KV;
  // this wave can skip tiles fully above its causal row range
  const int my_kv_end = causal ? min(S, qw0 + FA_QW) : S;
  // sliding window: tiles fully below ANY of this wave's rows' windows
  // are skipped; the whole WG starts at the block's earliest window tile
  const int my_kv_begin = window > 0 ? max(0, qw0 - window + 1) : 0;
  const int t_begin = window > 0 ? max(0, q0 - window + 1) / FA_KV : 0;

  const float s2 = scale * LOG2E;

  // ---- staging: the NR = 2 case of load_tile64 / write_tile64
  // (flash_common.h; same thread -> row/chunk map, same clamp-never-skip
  // rule), kept by hand: going through the helpers changes this kernel's
  // generated code (profiles/KERNEL_NOTES.md).  Thread t owns K/V rows
  // {2rp, 2rp+1} at 16-byte chunk c16 (rp = t>>4, c16 = t&15).
  const int tid = threadIdx.x;
  const int st_rp = tid >> 4;
  const int st_c16 = tid & 15;
  const int st_r0 = 2 * st_rp, st_r1 = 2 * st_rp + 1;

  uint4v kreg[2], vreg[2];
  auto issue_loads = [&](int t) {
    int kv0 = t * FA_KV;
    int rr0 = kv0 + st_r0 < S ? kv0 + st_r0 : S - 1;
    int rr1 = kv0 + st_r1 < S ? kv0 + st_r1 : S - 1;
    kreg[0] = *(const uint4v*)(kp + kv_base_k + (long)rr0 * k_ss + st_c16 * 8);
    kreg[1] = *(const uint4v*)(kp + kv_base_k + (long)rr1 * k_ss + st_c16 * 8);
    vreg[0] = *(const uint4v*)(vp + kv_base_v + (long)rr0 * v_ss + st_c16 * 8);
    vreg[1] = *(const uint4v*)(vp + kv_base_v + (long)rr1 * v_ss + st_c16 * 8);
  };

  auto write_tile = [&](int buf) {
    char* kimg = smem + buf * FA_BUF_B;
    char* vimg = kimg + FA_LDS_V;
    *(uint4v*)(kimg + img_off(st_r0, st_c16)) = kreg[0];
    *(uint4v*)(kimg + img_off(st_r1, st_c16)) = kreg[1];
    *(uint4v*)(vimg + img_off(st_r0, st_c16)) = vreg[0];
    *(uint4v*)(vimg + img_off(st_r1, st_c16)) = vreg[1];
  };

  // lane-dependent parts of the LDS read addresses (mfma.h): tile row `col`
  // for the K row reads, the 4x16 block pattern for the V transposed reads
  const int row_base = img_row_base(col, hi);
  const int tr_base = img_tr_base(lane) + FA_LDS_V;

  issue_loads(t_begin);
  write_tile(0);
  __syncthreads();
  // Q must have LANDED before the loop.  Left to itself the compiler sinks
  // the Q loads below the barrier and puts their vmcnt waits into the
  // loop's QK^T burst, where every iteration after the first they wait
  // for the NEXT tile's K/V loads issued a few instructions earlier: the
  // global latency the early issue is meant to hide.
#pragma unroll
  for (int c = 0; c < 8; ++c) asm volatile("" : "+v"(qf[c].u4));

  // Two staging buffers, ONE barrier per tile: tile t is read from buffer
  // `cur` while t+1 is written into cur^1 at the end of the iteration.  A
  // wave that gets there has passed the barrier that ended iteration t-1,
  // so every wave has finished reading cur^1 (tile t-1).
  int cur = 0;
  for (int t = t_begin; t < ntiles; ++t, cur ^= 1) {
    const int kv0 = t * FA_KV;
    if (t + 1 < ntiles) issue_loads(t + 1);

    // wave-uniform (wid is readfirstlane-derived, the rest kernel
    // arguments): the transposed reads below need all 64 lanes active
    const bool wave_active = kv0 < my_kv_end &&
        (window <= 0 || kv0 + FA_KV > my_kv_begin);
    if (wave_active) {
      const int rowb = row_base + cur * FA_BUF_B;
      const int trb = tr_base + cur * FA_BUF_B;
      // ---- QK^T: S^T[k][q] = sum_d K[k][d] Q^T[d][q] ------------------
      // All 16 K fragments are prefetched into registers BEFORE the mfma
      // burst (T3/T4): with ds_reads issued only 1-2 mfmas ahead the
      // compiler emits lgkmcnt(0) waits before every other mfma and the
      // ~64-cycle LDS latency stalls the matrix pipe; batching the reads
      // turns those into counted waits that are already satisfied.
      f32x16 acc[2] = {};
      frag_u kfr[2][8];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int c = 0; c < 8; ++c)
          kfr[kb][c].u4 =
              img_row_read(smem, rowb + kb * (32 * IMG_ROW_B), c);
      __builtin_amdgcn_s_setprio(1);  // T5: keep the matrix pipe fed
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int c = 0; c < 8; ++c)
          acc[kb] = mfma_bf16(kfr[kb][c].bf, qf[c].bf, acc[kb]);
      __builtin_amdgcn_s_setprio(0);

      // ---- V^T fragments of the whole tile: transposed reads of the V
      // image, vfr[c16][nb] = V[16*c16 + 8*hi + j][32*nb + col].  They take
      // over the registers the K fragments leave and land under the
      // softmax below.
      frag_u vfr[4][4];
#pragma unroll
      for (int c16 = 0; c16 < 4; ++c16)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          vfr[c16][nb].u4 = img_tr_read(smem, trb, 16 * c16, 32 * nb);

      // ---- online softmax (exp2 domain), lane-local per q row ---------
      float sc[2][16];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[kb][r] = acc[kb][r] * s2;
      const bool need_mask =
          (causal && kv0 + FA_KV > qw0) || (kv0 + FA_KV > S) ||
          (window > 0 && kv0 < qw0 + FA_QW - 1 - window + 1 + FA_KV);
      // (the branch holds only the selects; interior tiles skip it)
      if (need_mask) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            int kg = kv0 + 32 * kb + acc_row(r, hi);
            sc[kb][r] = fa_masked<false>(kg, my_q, S, causal, window)
                ? NEG_INF : sc[kb][r];
          }
      }

      float mt = NEG_INF;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, sc[kb][r]);
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));  // combine partner half

      float m_new = fmaxf(m_run, mt);
      // m_eff floor: when a lane's rows are ALL masked so far, m_new is
      // -1e30 and exp2(sc - m_new) would be exp2(0)=1 for masked scores;
      // the floor keeps those at exp2(-9.9e29) = 0.
      float m_eff = fmaxf(m_new, -1e28f);
      float alpha = __builtin_amdgcn_exp2f(m_run - m_eff);  // 0 when m_run=-1e30
      m_run = m_new;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) ot[nb] *= alpha;

      // ---- P = exp2(S - m) and its row sum; P chunk s (16 kv rows) is
      // packed to the bf16 B fragment pf[s] of the PV mfmas ---------------
      float psum = 0.f;
      frag_u pf[4];
      auto p_chunk = [&](int s) {
        const int kb = s >> 1, r0 = 8 * (s & 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float p = __builtin_amdgcn_exp2f(sc[kb][r0 + j] - m_eff);
          sc[kb][r0 + j] = p;
          psum += p;
        }
        pf[s] = acc8_to_frag(sc[kb], r0);
      };
      // ---- PV: O^T[d][q] += V^T[d][k] P^T[k][q] -----------------------
#pragma unroll
      for (int s = 0; s < 4; ++s) p_chunk(s);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int c16 = 0; c16 < 4; ++c16)
          ot[nb] = mfma_bf16(vfr[c16][nb].bf, pf[c16].bf, ot[nb]);
      __builtin_amdgcn_s_setprio(0);
      psum += __shfl_xor(psum, 32, 64);
      l_run = l_run * alpha + psum;
    }

    if (t + 1 < ntiles) write_tile(cur ^ 1);
    __syncthreads();
  }

  // ---- epilogue: normalize, store O (transposed back) and LSE ---------
  float inv_l = l_run > 0.f ? 1.f / l_run : 0.f;
  long o_base = (long)b * o_bs + (long)h * o_hs;
  // The loop's last barrier has passed, so the staging buffers are free:
  // each wave transposes its 32x128 O tile through 8 KB of them (image
  // rows = q rows) and stores whole 256-byte rows, 4 rows per b128 store
  // instruction, instead of 8 bytes per lane at a row stride.
  if (qw0 < S) {
    char* otile = smem + wid * (FA_QW * IMG_ROW_B);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        // d = 32*nb + 8*rg + 4*hi .. +3: chunk 4*nb + rg, half hi
        uint w0 = pack_bf16x2(ot[nb][4 * rg + 0] * inv_l,
                              ot[nb][4 * rg + 1] * inv_l);
        uint w1 = pack_bf16x2(ot[nb][4 * rg + 2] * inv_l,
                              ot[nb][4 * rg + 3] * inv_l);
        uint2 st = {w0, w1};
        *(uint2*)(otile + img_off(col, 4 * nb + rg) + 8 * hi) = st;
      }
    }
    __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int p = lane + i * 64;
      int row = p >> 4, c16 = p & 15;
      int qg = qw0 + row;
      if (qg < S) {
        uint4v vv = *(const uint4v*)(otile + img_off(row, c16));
        *(uint4v*)(op + o_base + (long)qg * o_ss + c16 * 8) = vv;
      }
    }
  }
  if (my_q >= S) return;
  if (hi == 0 && lsep) {
    // natural-log LSE: scores were in exp2 domain
    lsep[(long)(b * Hq + h) * S + my_q] =
        m_run * 0.6931471805599453f + __logf(l_run);
  }
}

extern "C" void flash_attn_fwd_strided(
    const void* q, const void* k, const void* v, void* out, void* lse,
    int B, int Hq, int Hkv, int S, float scale, int causal, int window,
    const long* st, hipStream_t stream) {
  // st = 12 longs: (bs, hs, ss) x (q, k, v, o)
  dim3 grid(Hq, (S + FA_QBLK - 1) / FA_QBLK, B);
  size_t lds = FA_LDS_TOTAL;
  flash_fwd_kernel<<<grid, 512, lds, stream>>>(
      (const short*)q, (const short*)k, (const short*)v, (short*)out,
      (float*)lse, B, Hq, Hkv, S, scale, causal, window,
      st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8],
      st[9], st[10], st[11]);
}

// dense (B, H, S, 128) entry points
extern "C" void flash_attn_fwd_window(const void* q, const void* k,
                                      const void* v, void* out, void* lse,
                                      int B, int Hq, int Hkv, int S,
                                      float scale, int window,
                                      hipStream_t stream) {
  long st[12];
  fa_dense_strides(st, Hq, Hkv, S);
  flash_attn_fwd_strided(q, k, v, out, lse, B, Hq, Hkv, S, scale, 1, window,
                         st, stream);
}

extern "C" void flash_attn_fwd(const void* q, const void* k, const void* v,
                               void* out, void* lse, int B, int Hq, int Hkv,
                               int S, float scale, int causal,
                               hipStream_t stream) {
  long st[12];
  fa_dense_strides(st, Hq, Hkv, S);
  flash_attn_fwd_strided(q, k, v, out, lse, B, Hq, Hkv, S, scale, causal, 0,
                         st, stream);
}
