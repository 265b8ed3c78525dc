// FlashAttention backward for CDNA4 (gfx950) — FA2-style recompute.
//
// Replaces the reference's NKI flash_attn_bwd (K2, SURVEY.md §2.3;
// reference kernels/flash_attn.py:18,76-88).  Three kernels:
//   * fa_bwd_delta: delta[q] = sum_d dO*O (rowwise fp32)
//   * fa_bwd_dkdv:  grid over 128-row KV blocks (4 waves x 32 kv rows);
//       sequential q-tile loop recomputes P^T from (Q,K,lse), forms
//       dS^T = P^T*(dP^T - delta), accumulates dK/dV in registers.
//       dK/dV written per Q-HEAD (B,Hq,S,D); the GQA reduction over the
//       Hq/Hkv replicas happens in the python wrapper.
//   * fa_bwd_dq:    grid over 128-row Q blocks (4 waves x 32 q rows);
//       sequential kv-tile loop, dQ accumulated in registers.
// No atomics anywhere: every output region is written by exactly one
// workgroup.
//
// Staging: every tile (Q, dO in dkdv; K, V in dq) is stored in LDS ONCE,
// in the dual-use image of mfma.h, and read both row-wise (ds_read_b128)
// and transposed (ds_read_b64_tr_b16).  Both kernels double-buffer the
// staged tiles.  LDS budget: dkdv 2 x 33,280 B staging + 32,768 B exchange
// = 99,328 B (1 WG/CU); dq 2 x 32,768 B = 65,536 B (2 WG/CU).
//
// Orientation trick shared with the forward kernel: all mfmas keep the
// softmax-normalized index (q) on the lane axis (col = l&31) so lse/delta
// are per-lane scalars; operands that need the other orientation go
// through small per-wave LDS tiles written from the accumulator layout.

#include "flash_common.h"

// ---------------------------------------------------------------------------
// delta = rowsum(dO * O)
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
fa_bwd_delta_kernel(const short* __restrict__ dout,
                    const short* __restrict__ out, float* __restrict__ delta,
                    long rows, int Hq, int S,
                    long do_bs, long do_hs, long do_ss,
                    long o_bs, long o_hs, long o_ss) {
  // row enumerates (b, h, s).  16 lanes own one 128-elem row (8 bf16 per
  // lane via b128 loads, coalesced 256 B per row segment); 4 shfl_xor
  // steps fold the 16 partials — no LDS, no block barrier.  This is a
  // pure streaming op (read 2 x B*Hq*S*128 bf16) and runs at HBM rate;
  // the previous one-block-per-row form was ~14x off the read floor.
  const int sub = threadIdx.x & 15;
  const long row0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const long row_step = ((long)gridDim.x * blockDim.x) >> 4;
  for (long row = row0; row < rows; row += row_step) {
    const long b = row / ((long)Hq * S);
    const long h = (row / S) % Hq;
    const long sq = row % S;
    s8v dv = *(const s8v*)(dout + b * do_bs + h * do_hs + sq * do_ss
                           + sub * 8);
    s8v ov = *(const s8v*)(out + b * o_bs + h * o_hs + sq * o_ss + sub * 8);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += bits2f(dv[j]) * bits2f(ov[j]);
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (sub == 0) delta[row] = s;
  }
}

// ---------------------------------------------------------------------------
// dK/dV kernel (8 waves over a 128-row kv block; see kernel comment)
// LDS: 2 staging buffers x {Q 16 KB + dO 16 KB + lse/delta 512 B} = 65 KB
// + 32 KB cross-wave exchange = 97 KB -- the P/dS tiles live entirely in
// registers (pack + permlane32_swap repack).
// ---------------------------------------------------------------------------
#define BW64_BUF_B (2 * TILE64_B + 128 * 4)   // 33280 B per staging buffer
#define BW64_LDS_Q 0
#define BW64_LDS_DO TILE64_B
// 128 floats: lse*log2(e) for the 64 q rows at [0..64), delta at [64..128)
#define BW64_LDS_LD (2 * TILE64_B)
// cross-wave A-fragment exchange: 8 slots (kvg x q-half) x 4 frags x
// 64 lanes x 16 B = 32 KB.  The kernel is VGPR-bound at 1 WG/CU (2
// waves/SIMD), so this LDS is free occupancy-wise.
#define BW64_LDS_X (2 * BW64_BUF_B)
#define BW64_X_SLOT(kvg, half, f) \
  ((((kvg) * 2 + (half)) * 4 + (f)) * 64 * 16)
#define BW64_LDS_TOTAL (BW64_LDS_X + 8 * 4 * 64 * 16)   // 99328 B

extern "C" __global__ void __launch_bounds__(512, 2)
fa_bwd_dkdv_kernel(const short* __restrict__ qp, const short* __restrict__ kp,
                   const short* __restrict__ vp,
                   const short* __restrict__ dop,
                   const float* __restrict__ lsep,
                   const float* __restrict__ deltap,
                   short* __restrict__ dkp, short* __restrict__ dvp,
                   int B, int Hq, int Hkv, int S, float scale, int causal,
                   int window,
                   long q_bs, long q_hs, long q_ss,
                   long k_bs, long k_hs, long k_ss,
                   long v_bs, long v_hs, long v_ss,
                   long do_bs, long do_hs, long do_ss,
                   long dk_bs, long dk_hs, long dk_ss,
                   long dv_bs, long dv_hs, long dv_ss) {
  // 8 waves / 128-row kv block: wave w -> kv rows (w>>1)*32, d-half w&1.
  // Q-TILE = 64 rows per iteration, processed as two 32-q halves that
  // REUSE the st/dpt accumulators: one barrier pair and one staging round
  // per 64 q rows.
  //
  // The score/dS tiles never touch LDS: S^T/dP are computed with Q on the
  // A operand (q in accumulator REGISTER rows, kv in lanes), so the
  // register repack (acc8_to_frag, flash_common.h) turns them directly into the A fragments of the dV/dK mfmas (k-dim = q,
  // lane = kv).  The softmax's per-q lse/delta become per-register-row
  // values read from a 128-float LDS tile staged once per q-tile.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  // readfirstlane: provably wave-uniform -> scalar branches for the
  // per-wave activity guards instead of exec-mask divergence (T20)
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 31;
  const int hi = lane >> 5;
  const int kvg = wid >> 1;        // kv row group 0..3
  const int dhalf = wid & 1;       // d half 0..1

  // heads on x, kv-blocks on y: causal work DEcreases with kv-block index,
  // so ascending y already dispatches biggest-first (greedy LPT; see the
  // fwd kernel's dispatch note)
  const int kvblk = blockIdx.y;
  const int h = blockIdx.x;
  const int b = blockIdx.z;
  const int hkv = h / (Hq / Hkv);
  const long q_base = (long)b * q_bs + (long)h * q_hs;
  const long do_base = (long)b * do_bs + (long)h * do_hs;
  const long k_base = (long)b * k_bs + (long)hkv * k_hs;
  const long v_base = (long)b * v_bs + (long)hkv * v_hs;
  const long lse_base = (long)(b * Hq + h) * S;

  const int kv0 = kvblk * 128 + kvg * 32;   // this wave's kv rows
  const int my_k = kv0 + col;

  frag_u kf[8], vf[8];
  {
    int row = my_k < S ? my_k : S - 1;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      kf[c].u4 = *(const uint4v*)(kp + k_base + (long)row * k_ss + c * 16 + hi * 8);
      vf[c].u4 = *(const uint4v*)(vp + v_base + (long)row * v_ss + c * 16 + hi * 8);
    }
  }

  f32x16 dv_acc[2] = {};
  f32x16 dk_acc[2] = {};

  // threads 0..63 fetch lse (pre-scaled by log2 e), 64..127 delta
  auto load_ld = [&](int qt0) -> float {
    int qg = qt0 + (threadIdx.x & 63);
    int qc = qg < S ? qg : S - 1;
    if (threadIdx.x < 64) return lsep[lse_base + qc] * LOG2E;
    if (threadIdx.x < 128) return deltap[lse_base + qc];
    return 0.f;
  };
  auto write_ld = [&](float v, char* buf) {
    if (threadIdx.x < 128) ((float*)(buf + BW64_LDS_LD))[threadIdx.x] = v;
  };

  const float s2 = scale * LOG2E;
  int q_start = causal ? kvblk * 128 : 0;
  // sliding window: q attends k iff k <= q < k + window, so this kv
  // block's active q rows end at kv_max + window
  int q_end = S;
  if (window > 0) {
    int qe = kvblk * 128 + 127 + window;
    q_end = qe < S ? qe : S;
  }

  write_tile64(load_tile64<2>(qp + q_base, q_start, q_ss, S - q_start),
               smem + BW64_LDS_Q);
  write_tile64(load_tile64<2>(dop + do_base, q_start, do_ss, S - q_start),
               smem + BW64_LDS_DO);
  write_ld(load_ld(q_start), smem);

  // Two staging buffers, two barriers per 64 q rows:
  //   barrier A: buffer `cur` (written during the previous iteration) is
  //     visible, and every wave has finished the previous consume, so the
  //     exchange slots and buffer cur^1 are free;
  //   barrier B: the produced A fragments are visible.
  // The next tile's global loads are issued right after A and land in
  // buffer cur^1 after the consume — nobody reads that buffer before the
  // next barrier A, so no third barrier is needed.
  // lane-dependent parts of the LDS read addresses (mfma.h): tile row
  // `col` for the row reads; this wave's d-half (a 128-byte, i.e.
  // 8-chunk, column offset: an XOR on the chunk index) for the transposed
  // reads
  const int row_base = img_row_base(col, hi);
  const int tr_base = img_tr_base(lane) ^ (dhalf * 128);
  StageRegs<2> nq, ndo;
  float nld = 0.f;
  int cur = 0;
  for (int q0 = q_start; q0 < q_end; q0 += 64, cur ^= 1) {
    const int sb_off = cur * BW64_BUF_B;
    const float* ld_sm = (const float*)(smem + sb_off + BW64_LDS_LD);
    const int rowb = row_base + sb_off;
    const int trb = tr_base + sb_off;
    __syncthreads();
    if (q0 + 64 < q_end) {
      nq = load_tile64<2>(qp + q_base, q0 + 64, q_ss, S - q0 - 64);
      ndo = load_tile64<2>(dop + do_base, q0 + 64, do_ss, S - q0 - 64);
      nld = load_ld(q0 + 64);
    }
    // ---- PRODUCE: this wave computes S^T/dP^T for q-half = dhalf ONLY.
    // Its dhalf-partner wave (same kvg) computes the other half; the
    // packed A fragments are exchanged through LDS, halving the score
    // mfma work per wave (the old form had both waves of a kvg pair
    // redo the identical full-d S^T/dP^T for both halves: 48 mfmas per
    // wave-iteration where 32 are algorithmically needed — measured as
    // dkdv running at 363 TF vs the forward's 533).
    {
      const int half = dhalf;
      const int qh0 = q0 + half * 32;
      const bool produce =
          (!causal || (qh0 + 31 >= kv0)) && qh0 < S &&
          (window <= 0 || qh0 < kv0 + 31 + window);
      if (produce) {
        const int my_kv = kv0 + col;         // this lane's kv column

        // S^T2[q][kv]: A = Q rows (B-layout frag doubles as A: lane=q),
        // B = K rows (lane=kv) -> q in accumulator rows, kv in lanes
        f32x16 st = {};
        f32x16 dpt = {};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          frag_u qfr, dofr;
          qfr.u4 = img_row_read(smem + BW64_LDS_Q, rowb + half * (32 * IMG_ROW_B), c);
          st = mfma_bf16(qfr.bf, kf[c].bf, st);
          dofr.u4 = img_row_read(smem + BW64_LDS_DO, rowb + half * (32 * IMG_ROW_B), c);
          dpt = mfma_bf16(dofr.bf, vf[c].bf, dpt);
        }

        // p / dS per element; lse & delta indexed by the REGISTER q row.
        // acc rows r = 4g..4g+3 are CONSECUTIVE q rows 8g+4*hi.. so the
        // 32 per-row values batch into 8 b128 broadcast reads (one wait)
        // instead of 32 serialized b32 reads.
        float lse_v[16], dlt_v[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          *(float4*)(lse_v + 4 * g) =
              *(const float4*)(ld_sm + half * 32 + 8 * g + 4 * hi);
          *(float4*)(dlt_v + 4 * g) =
              *(const float4*)(ld_sm + 64 + half * 32 + 8 * g + 4 * hi);
        }
        // wave-uniform (as in the forward kernel): the 32q x 32kv sub-tile
        // needs the per-element predicate only if it touches the causal
        // diagonal, the end of the sequence or the window's band edge;
        // interior tiles skip it
        const bool need_mask =
            (causal && kv0 + 31 > qh0) || kv0 + 31 >= S || qh0 + 31 >= S ||
            (window > 0 && qh0 + 31 >= kv0 + window);
        // (the branch holds only the selects that zero masked p's: two
        // full copies of the p/dS loop made the register allocator spill)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          st[r] = __builtin_amdgcn_exp2f(st[r] * s2 - lse_v[r]);
        if (need_mask) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            int ql = half * 32 + acc_row(r, hi);
            int qg = q0 + ql;
            // fa_masked<true>(my_kv, qg, ...) written out, with the window
            // term from the kv side: the helper changes this kernel's
            // generated code (profiles/KERNEL_NOTES.md)
            bool masked = ((causal != 0) & (my_kv > qg)) | (my_kv >= S) |
                (qg >= S) | ((window > 0) & (qg >= my_kv + window));
            st[r] = masked ? 0.f : st[r];
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) dpt[r] = st[r] * (dpt[r] - dlt_v[r]);

        // repack accumulator rows (q) into A-fragment k-dim in REGISTERS
        // (lane dim = kv is already in place).  This is acc8_to_frag
        // (flash_common.h) written out for st and dpt: calling the helper
        // here changes this kernel's generated code
        // (profiles/KERNEL_NOTES.md).
        frag_u pA[2], dA[2];
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          uint b0 = pack_bf16x2(st[8 * cc + 0], st[8 * cc + 1]);
          uint b1 = pack_bf16x2(st[8 * cc + 2], st[8 * cc + 3]);
          uint b2 = pack_bf16x2(st[8 * cc + 4], st[8 * cc + 5]);
          uint b3 = pack_bf16x2(st[8 * cc + 6], st[8 * cc + 7]);
          {
            auto r01 = __builtin_amdgcn_permlane32_swap(b0, b2, false, false);
            b0 = r01[0]; b2 = r01[1];
          }
          {
            auto r23 = __builtin_amdgcn_permlane32_swap(b1, b3, false, false);
            b1 = r23[0]; b3 = r23[1];
          }
          pA[cc].u[0] = b0; pA[cc].u[1] = b1;
          pA[cc].u[2] = b2; pA[cc].u[3] = b3;
          uint c0 = pack_bf16x2(dpt[8 * cc + 0], dpt[8 * cc + 1]);
          uint c1 = pack_bf16x2(dpt[8 * cc + 2], dpt[8 * cc + 3]);
          uint c2 = pack_bf16x2(dpt[8 * cc + 4], dpt[8 * cc + 5]);
          uint c3 = pack_bf16x2(dpt[8 * cc + 6], dpt[8 * cc + 7]);
          {
            auto r01 = __builtin_amdgcn_permlane32_swap(c0, c2, false, false);
            c0 = r01[0]; c2 = r01[1];
          }
          {
            auto r23 = __builtin_amdgcn_permlane32_swap(c1, c3, false, false);
            c1 = r23[0]; c3 = r23[1];
          }
          dA[cc].u[0] = c0; dA[cc].u[1] = c1;
          dA[cc].u[2] = c2; dA[cc].u[3] = c3;
        }

        // publish this half's A fragments for both d-half waves of the
        // kvg pair (frag-major layout: consecutive lanes x 16 B ->
        // conflict-free ds_write_b128)
        char* xb = smem + BW64_LDS_X;
        *(uint4v*)(xb + BW64_X_SLOT(kvg, half, 0) + lane * 16) = pA[0].u4;
        *(uint4v*)(xb + BW64_X_SLOT(kvg, half, 1) + lane * 16) = pA[1].u4;
        *(uint4v*)(xb + BW64_X_SLOT(kvg, half, 2) + lane * 16) = dA[0].u4;
        *(uint4v*)(xb + BW64_X_SLOT(kvg, half, 3) + lane * 16) = dA[1].u4;
      }
    }
    __syncthreads();  // exchange visible

    // ---- CONSUME: both q halves on this wave's 64-column d-half -------
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int qh0 = q0 + half * 32;
      if ((causal && qh0 + 31 < kv0) || qh0 >= S ||
          (window > 0 && qh0 >= kv0 + 31 + window)) continue;

      // prefetch the dV/dK B fragments first — independent of the slot
      // reads, so all LDS loads pipeline into one counted wait.  They are
      // transposed reads of the SAME image the producer reads row-wise;
      // the guard above is wave-uniform, so all 64 lanes are active here.
      frag_u dofr[2][2], qfr2[2][2];
#pragma unroll
      for (int cq = 0; cq < 2; ++cq)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          dofr[cq][nb].u4 = img_tr_read(smem + BW64_LDS_DO, trb,
                                        half * 32 + cq * 16, nb * 32);
          qfr2[cq][nb].u4 = img_tr_read(smem + BW64_LDS_Q, trb,
                                        half * 32 + cq * 16, nb * 32);
        }
      frag_u pA[2], dA[2];
      const char* xb = smem + BW64_LDS_X;
      pA[0].u4 = *(const uint4v*)(xb + BW64_X_SLOT(kvg, half, 0) + lane * 16);
      pA[1].u4 = *(const uint4v*)(xb + BW64_X_SLOT(kvg, half, 1) + lane * 16);
      dA[0].u4 = *(const uint4v*)(xb + BW64_X_SLOT(kvg, half, 2) + lane * 16);
      dA[1].u4 = *(const uint4v*)(xb + BW64_X_SLOT(kvg, half, 3) + lane * 16);

      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int cq = 0; cq < 2; ++cq)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          dv_acc[nb] = mfma_bf16(pA[cq].bf, dofr[cq][nb].bf, dv_acc[nb]);
          dk_acc[nb] = mfma_bf16(dA[cq].bf, qfr2[cq][nb].bf, dk_acc[nb]);
        }
      __builtin_amdgcn_s_setprio(0);
    }

    if (q0 + 64 < q_end) {
      char* nxt = smem + (cur ^ 1) * BW64_BUF_B;
      write_tile64(nq, nxt + BW64_LDS_Q);
      write_tile64(ndo, nxt + BW64_LDS_DO);
      write_ld(nld, nxt);
    }
  }

  // ---- epilogue: per-wave 32x64 halves via LDS transpose ---------------
  __syncthreads();
  char* otile = smem + wid * (32 * 64 * 2);  // 4 KB per wave
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int k = acc_row(r, hi);
      int dd = nb * 32 + col;
      *(short*)(otile + (k * 64 + dd) * 2) = f2bits(dv_acc[nb][r]);
    }
  __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int p = lane + i * 64;
    int row = p >> 3, c16 = p & 7;
    int kg = kv0 + row;
    if (kg < S) {
      uint4v vv = *(const uint4v*)(otile + (row * 64 + c16 * 8) * 2);
      *(uint4v*)(dvp + (long)b * dv_bs + (long)h * dv_hs
                 + (long)kg * dv_ss + dhalf * 64
                 + c16 * 8) = vv;
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int k = acc_row(r, hi);
      int dd = nb * 32 + col;
      *(short*)(otile + (k * 64 + dd) * 2) = f2bits(dk_acc[nb][r] * scale);
    }
  __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int p = lane + i * 64;
    int row = p >> 3, c16 = p & 7;
    int kg = kv0 + row;
    if (kg < S) {
      uint4v vv = *(const uint4v*)(otile + (row * 64 + c16 * 8) * 2);
      *(uint4v*)(dkp + (long)b * dk_bs + (long)h * dk_hs
                 + (long)kg * dk_ss + dhalf * 64
                 + c16 * 8) = vv;
    }
  }
}

// ---------------------------------------------------------------------------
// dQ kernel: 4 waves, wave owns q rows [q0 + 32*wid, +32)
// LDS: 2 staging buffers x {K 16 KB + V 16 KB} (64-row kv tiles) = 64 KB;
// the epilogue's 4 per-wave 32x128 transpose tiles (32 KB) reuse it.
// 2 WG/CU -> 128 KB of the CU's 160 KB.
// ---------------------------------------------------------------------------
#define DQ_BUF_B (2 * TILE64_B)   // 32768 B per staging buffer
#define DQ_LDS_K 0
#define DQ_LDS_V TILE64_B
#define DQ_LDS_TOTAL (2 * DQ_BUF_B)   // 65536 B

extern "C" __global__ void __launch_bounds__(256, 2)
fa_bwd_dq_kernel(const short* __restrict__ qp, const short* __restrict__ kp,
                 const short* __restrict__ vp, const short* __restrict__ dop,
                 const float* __restrict__ lsep,
                 const float* __restrict__ deltap, short* __restrict__ dqp,
                 int B, int Hq, int Hkv, int S, float scale, int causal,
                 int window,
                 long q_bs, long q_hs, long q_ss,
                 long k_bs, long k_hs, long k_ss,
                 long v_bs, long v_hs, long v_ss,
                 long do_bs, long do_hs, long do_ss,
                 long dq_bs, long dq_hs, long dq_ss) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  // readfirstlane: provably wave-uniform -> scalar branches for the
  // per-wave activity guards instead of exec-mask divergence (T20)
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 31;
  const int hi = lane >> 5;

  // heads on x, q-blocks on y reversed: biggest-causal-work first (LPT,
  // see the fwd kernel's dispatch note)
  const int qblk = (int)(gridDim.y - 1 - blockIdx.y);
  const int h = blockIdx.x;
  const int b = blockIdx.z;
  const int hkv = h / (Hq / Hkv);
  const long q_base = (long)b * q_bs + (long)h * q_hs;
  const long do_base = (long)b * do_bs + (long)h * do_hs;
  const long dq_base = (long)b * dq_bs + (long)h * dq_hs;
  const long k_base = (long)b * k_bs + (long)hkv * k_hs;
  const long v_base = (long)b * v_bs + (long)hkv * v_hs;
  const long lse_base = (long)(b * Hq + h) * S;

  const int q0 = qblk * 128 + wid * 32;
  const int my_q = q0 + col;
  const int q_ld = my_q < S ? my_q : S - 1;

  // Q, dO fragments in registers (lane: row q=col within wave tile)
  frag_u qf[8], dof[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    qf[c].u4 = *(const uint4v*)(qp + q_base + (long)q_ld * q_ss + c * 16 + hi * 8);
    dof[c].u4 = *(const uint4v*)(dop + do_base + (long)q_ld * do_ss + c * 16 + hi * 8);
  }
  const float lse2 = lsep[lse_base + q_ld] * LOG2E;
  const float dlt = deltap[lse_base + q_ld];

  f32x16 dq_acc[4] = {};

  // WG-uniform loop bound (all waves share barriers); per-wave causal
  // skipping happens via wave_active below
  const int kv_end = causal ? min(S, qblk * 128 + 128) : S;
  // sliding window: this q block's earliest active kv row (tile-aligned)
  const int kv_begin = window > 0
      ? ((qblk * 128 - window + 1 > 0 ? qblk * 128 - window + 1 : 0) & ~31)
      : 0;
  const float s2 = scale * LOG2E;

  write_tile64(load_tile64<4>(kp + k_base, kv_begin, k_ss, S - kv_begin),
               smem + DQ_LDS_K);
  write_tile64(load_tile64<4>(vp + v_base, kv_begin, v_ss, S - kv_begin),
               smem + DQ_LDS_V);

  // 64-row kv tiles in two staging buffers, ONE barrier per tile: it makes
  // buffer `cur` visible and guarantees every wave has left buffer cur^1
  // (read during the previous iteration), which this iteration refills
  // after its compute.  Each tile is consumed as two 32-row halves in
  // ascending kv order, so dq_acc accumulates in the same order as with
  // 32-row tiles.
  const int row_base = img_row_base(col, hi);
  const int tr_base = img_tr_base(lane);
  StageRegs<4> nk, nv;
  int cur = 0;
  for (int kv0 = kv_begin; kv0 < kv_end; kv0 += 64, cur ^= 1) {
    const int rowb = row_base + cur * DQ_BUF_B;
    const int trb = tr_base + cur * DQ_BUF_B;
    __syncthreads();
    if (kv0 + 64 < kv_end) {
      nk = load_tile64<4>(kp + k_base, kv0 + 64, k_ss, S - kv0 - 64);
      nv = load_tile64<4>(vp + v_base, kv0 + 64, v_ss, S - kv0 - 64);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int kvh0 = kv0 + half * 32;
      // all guards here are wave-uniform (loop bounds and q0 come from
      // scalars / readfirstlane): the transposed reads below need all 64
      // lanes active
      const bool wave_active = kvh0 < kv_end &&
          (!causal || (kvh0 <= q0 + 31)) &&
          (window <= 0 || kvh0 + 31 + window > q0);
      if (!wave_active) continue;

      // S^T[k][q]: A = K rows (LDS image, row k=col), B = Q^T (regs)
      f32x16 st = {};
      f32x16 dpt = {};
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        frag_u kfr;
        kfr.u4 = img_row_read(smem + DQ_LDS_K, rowb + half * (32 * IMG_ROW_B), c);
        st = mfma_bf16(kfr.bf, qf[c].bf, st);
        frag_u vfr;
        vfr.u4 = img_row_read(smem + DQ_LDS_V, rowb + half * (32 * IMG_ROW_B), c);
        dpt = mfma_bf16(vfr.bf, dof[c].bf, dpt);
      }

      // wave-uniform: the per-element predicate is needed only when the
      // 32kv x 32q sub-tile touches the causal diagonal, the end of the
      // sequence or the window's band edge
      const bool need_mask =
          (causal && kvh0 + 31 > q0) || kvh0 + 31 >= S || q0 + 31 >= S ||
          (window > 0 && kvh0 <= q0 + 31 - window);
      // (the branch holds only the selects that zero masked p's, which
      // keeps register pressure where it was)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        st[r] = __builtin_amdgcn_exp2f(st[r] * s2 - lse2);
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int kg = kvh0 + acc_row(r, hi);
          st[r] = fa_masked<true>(kg, my_q, S, causal, window) ? 0.f : st[r];
        }
      }
      f32x16 dst;
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[r] = st[r] * (dpt[r] - dlt);

      // prefetch the 8 K B-fragments (independent of the pack below — the
      // LDS reads land under the pack VALU): transposed reads of the same
      // K image the S^T mfmas read row-wise
      frag_u kfr2[2][4];
#pragma unroll
      for (int ck = 0; ck < 2; ++ck)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          kfr2[ck][nb].u4 = img_tr_read(smem + DQ_LDS_K, trb,
                                        half * 32 + ck * 16, nb * 32);

      // repack dS accumulator rows (kv) into A-fragment k-dim in
      // REGISTERS (lane dim q already in place)
      frag_u dA[2];
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) dA[cc] = acc8_to_frag(dst, 8 * cc);

      // dQ[q][d] += sum_k dS[q][k] K[k][d]
      //   A = dS (registers, lane=q), B = K[k][d] (transposed reads)
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ck = 0; ck < 2; ++ck) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          dq_acc[nb] = mfma_bf16(dA[ck].bf, kfr2[ck][nb].bf, dq_acc[nb]);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    if (kv0 + 64 < kv_end) {
      char* nxt = smem + (cur ^ 1) * DQ_BUF_B;
      write_tile64(nk, nxt + DQ_LDS_K);
      write_tile64(nv, nxt + DQ_LDS_V);
    }
  }

  // epilogue: dQ (col = d, rows q) -> LDS transpose -> coalesced store
  __syncthreads();
  char* otile = smem + wid * (32 * FA_D * 2);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int qr = acc_row(r, hi);
      int d = nb * 32 + col;
      *(short*)(otile + (qr * FA_D + d) * 2) = f2bits(dq_acc[nb][r] * scale);
    }
  __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int p = lane + i * 64;
    int row = p >> 4, c16 = p & 15;
    int qg = q0 + row;
    if (qg < S) {
      uint4v vv = *(const uint4v*)(otile + (row * FA_D + c16 * 8) * 2);
      *(uint4v*)(dqp + dq_base + (long)qg * dq_ss + c16 * 8) = vv;
    }
  }
}

// ---------------------------------------------------------------------------
extern "C" void flash_attn_bwd_strided(
    const void* q, const void* k, const void* v, const void* out,
    const void* dout, const void* lse, void* delta, void* dq, void* dk,
    void* dv, int B, int Hq, int Hkv, int S, float scale, int causal,
    int window, const long* st, hipStream_t stream) {
  // st = 24 longs: (bs, hs, ss) x (q, k, v, o, dout, dq, dk, dv)
  long rows = (long)B * Hq * S;
  // 16 lanes per row -> 16 rows per 256-thread block; cap well above the
  // 256-CU fill point and grid-stride the rest
  long blocks = (rows + 15) / 16;
  int nb = blocks < 8192 ? (int)blocks : 8192;
  fa_bwd_delta_kernel<<<nb, 256, 0, stream>>>(
      (const short*)dout, (const short*)out, (float*)delta, rows, Hq, S,
      st[12], st[13], st[14], st[9], st[10], st[11]);
  dim3 gkv(Hq, (S + 127) / 128, B);
  // 2 staging buffers (2 x 33,280 B) + A-fragment exchange (32,768 B) =
  // 99,328 B; the kernel is VGPR-bound at 1 WG/CU so the LDS costs no
  // occupancy
  size_t lds1 = BW64_LDS_TOTAL;
  fa_bwd_dkdv_kernel<<<gkv, 512, lds1, stream>>>(
      (const short*)q, (const short*)k, (const short*)v, (const short*)dout,
      (const float*)lse, (const float*)delta, (short*)dk, (short*)dv, B, Hq,
      Hkv, S, scale, causal, window, st[0], st[1], st[2], st[3], st[4],
      st[5], st[6], st[7], st[8], st[12], st[13], st[14], st[18], st[19],
      st[20], st[21], st[22], st[23]);
  dim3 gq(Hq, (S + 127) / 128, B);
  // 2 staging buffers x (K + V 64-row tiles) = 64 KB; the epilogue's 4
  // per-wave 32x128 transpose tiles (32 KB) reuse it.  64 KB keeps 2 WG/CU.
  size_t lds2 = DQ_LDS_TOTAL;
  fa_bwd_dq_kernel<<<gq, 256, lds2, stream>>>(
      (const short*)q, (const short*)k, (const short*)v, (const short*)dout,
      (const float*)lse, (const float*)delta, (short*)dq, B, Hq, Hkv, S,
      scale, causal, window, st[0], st[1], st[2], st[3], st[4], st[5],
      st[6], st[7], st[8], st[12], st[13], st[14], st[15], st[16],
      st[17]);
}

extern "C" void flash_attn_bwd(const void* q, const void* k, const void* v,
                               const void* out, const void* dout,
                               const void* lse, void* delta, void* dq,
                               void* dk, void* dv, int B, int Hq, int Hkv,
                               int S, float scale, int causal,
                               hipStream_t stream) {
  long st[24];
  fa_dense_strides(st, Hq, Hkv, S);
  // dout, dq, dk, dv are q-shaped (dk/dv are per-Q-head buffers)
  for (int i = 12; i < 24; ++i) st[i] = st[i % 3];
  flash_attn_bwd_strided(q, k, v, out, dout, lse, delta, dq, dk, dv, B, Hq,
                         Hkv, S, scale, causal, 0, st, stream);
}
