// Fused decode attention for CDNA4: RoPE(q,k) + KV-cache append +
// flash-decode over the cache, GQA-grouped, split-KV two-phase.
//
// Performance history at the llama3-8b decode shape (B=32, Hkv=8,
// pos~1k; cache-read floor ~17 us):
//   v1  4 waves/WG, lane-per-2-dims, 6-step wave shuffle per row: 171 us
//   v2  16 waves + prefetch:                                       70 us
//   v3  + split-KV x4 two-phase:                                   80 us
//       (ablation: shuffle reduction ~32 us of it -> the ds-pipe
//        __shfl chain, not memory, was the wall)
//   v6  THIS: each 16-lane QUARTER-wave owns a row (8 dims/lane,
//       b128 loads), so the score reduction is 4 xor steps serving 4
//       rows per instruction, exp2 runs once per score, and a wave
//       retires 4 rows/iteration:                                  31 us
//
// Phase 1 (decode_attn_part): WG (b, kvh, split s) flash-decodes its
// pos/DA_SPLIT row chunk, merges its quarter-wave partials in LDS, writes
// one fp32 partial (m, l, o[REP][128]) to workspace; split 0 also
// appends the new K/V row and adds its term.  Phase 2
// (decode_attn_merge) log-sum-exp-combines the splits -> bf16 out; it is
// also phase 2 of decode_attn_mx.hip and, with T tokens, of chunk_attn.hip.
//
// Constants, layouts and every phase-1 piece but the walk over the cache
// are in decode_attn_common.h, shared with decode_attn_mx.hip.
// kcache/vcache are bf16 (B, Hkv, Smax, D).
//
// decode_attn takes one device position for the batch; decode_attn_ragged
// takes one per sequence (decode_attn_common.h, RAGGED).

#include "decode_attn_common.h"
#include "mfma.h"

template <int REP, bool RAGGED>
__global__ void __launch_bounds__(DA_WAVES * 64)
decode_attn_part(const short* __restrict__ qlin,
                    const short* __restrict__ klin,
                    const short* __restrict__ vlin,
                    short* __restrict__ kcache, short* __restrict__ vcache,
                    const float* __restrict__ cosp,
                    const float* __restrict__ sinp,
                    const long* __restrict__ pos_ptr,
                    float* __restrict__ part_o, float* __restrict__ part_ml,
                    int B, int Hq, int Hkv, int Smax, float scale,
                    int qstride, int kvstride) {
  DaCoord c;
  da_coord<REP, RAGGED>(c, pos_ptr, Hkv);
  if (RAGGED && !da_active(c.pos, 1, Smax)) {  // the whole workgroup
    da_store_neutral(c.wg, REP, DA_WAVES * 64, part_o, part_ml);
    return;
  }
  const int tid = c.tid, hl = c.hl;

  __shared__ float qr[REP][DA_D];
  __shared__ float knr[DA_D];
  __shared__ float vn[DA_D];
  __shared__ float merge_o[DA_SLOTS + 1][REP][DA_D];
  __shared__ float merge_ml[DA_SLOTS + 1][REP][2];

  // every split ropes the new k and loads v; only split 0 uses them
  if (tid < 64) {
    const float cs = cosp[c.pos * (DA_D / 2) + tid];
    const float sn = sinp[c.pos * (DA_D / 2) + tid];
    da_rope_q<REP>(qlin, qstride, c, cs, sn, qr);
    da_rope_pair(klin, (long)c.b * kvstride + c.kvh * DA_D, tid, cs, sn,
                 knr[tid], knr[tid + 64]);
  } else if (tid < 128) {
    int i = tid - 64;
    vn[i] = bits2f(vlin[(long)c.b * kvstride + c.kvh * DA_D + i]);
    vn[i + 64] = bits2f(vlin[(long)c.b * kvstride + c.kvh * DA_D + i + 64]);
  }
  __syncthreads();

  if (c.s == 0 && tid < DA_D) {
    const long cache_row = (((long)c.b * Hkv + c.kvh) * Smax + c.pos) * DA_D;
    kcache[cache_row + tid] = f2bits(knr[tid]);
    vcache[cache_row + tid] = f2bits(vn[tid]);
  }

  const short* kc = kcache + ((long)c.b * Hkv + c.kvh) * Smax * DA_D;
  const short* vc = vcache + ((long)c.b * Hkv + c.kvh) * Smax * DA_D;
  const float s2 = scale * DA_LOG2E;
  float qv[REP][8], m_run[REP], l_run[REP], ov[REP][8];
  da_init_state<REP>(qr, hl, qv, m_run, l_run, ov);

  // row quad per wave-iteration: row = base + wid*4 + quarter
  const long r1 = c.r1;
  long r = c.r0 + 4 * c.wid + c.quarter;
  const long rstep = DA_SLOTS;
  uint4v kp = {0, 0, 0, 0}, vp = {0, 0, 0, 0};
  if (r < r1) {
    kp = *(const uint4v*)(kc + r * DA_D + 8 * hl);
    vp = *(const uint4v*)(vc + r * DA_D + 8 * hl);
  }
  for (; r < r1;) {
    const long rn = r + rstep;
    uint4v kpn = {0, 0, 0, 0}, vpn = {0, 0, 0, 0};
    if (rn < r1) {
      kpn = *(const uint4v*)(kc + rn * DA_D + 8 * hl);
      vpn = *(const uint4v*)(vc + rn * DA_D + 8 * hl);
    }
    float kf[8], vf[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      kf[2 * j] = bits2f((short)(kp[j] & 0xffff));
      kf[2 * j + 1] = bits2f((short)(kp[j] >> 16));
      vf[2 * j] = bits2f((short)(vp[j] & 0xffff));
      vf[2 * j + 1] = bits2f((short)(vp[j] >> 16));
    }
    float part[REP];
#pragma unroll
    for (int g = 0; g < REP; ++g) {
      part[g] = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) part[g] += qv[g][j] * kf[j];
    }
    da_quarter_reduce<REP>(part);
#pragma unroll
    for (int g = 0; g < REP; ++g) {
      float sc = part[g] * s2;
      float m_new = fmaxf(m_run[g], sc);
      float alpha = __builtin_amdgcn_exp2f(m_run[g] - m_new);
      float p = __builtin_amdgcn_exp2f(sc - m_new);
      m_run[g] = m_new;
      l_run[g] = l_run[g] * alpha + p;
#pragma unroll
      for (int j = 0; j < 8; ++j) ov[g][j] = ov[g][j] * alpha + p * vf[j];
    }
    r = rn;
    kp = kpn;
    vp = vpn;
  }

  da_store_partial<REP>(c, ov, m_run, l_run, merge_o, merge_ml);
  if (c.s == 0 && c.wid == 0)
    da_new_row_term<REP>(c, qv, knr, vn, s2, merge_o, merge_ml);
  __syncthreads();
  da_merge_store<REP>(c, merge_o, merge_ml, part_o, part_ml);
}

// Phase 2, block (pair, token): wave w takes heads w, w + 4, a lane 2 dims of
// workspace row rho = tok * REP + g of each split.
template <int REP>
__global__ void __launch_bounds__(256)
decode_attn_merge(const float* __restrict__ part_o,
                  const float* __restrict__ part_ml, short* __restrict__ outp,
                  int T, int Hq, int Hkv) {
  const int pair = blockIdx.x;
  const int tok = blockIdx.y;
  const int kvh = pair % Hkv;
  const int b = pair / Hkv;
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int R = REP * T;
  for (int g = wid; g < REP; g += 4) {
    const int rho = tok * REP + g;
    float m_g = DA_NEG;
#pragma unroll
    for (int sp = 0; sp < DA_SPLIT; ++sp)
      m_g = fmaxf(m_g, part_ml[(((long)pair * DA_SPLIT + sp) * R + rho) * 2]);
    float l_g = 0.f, a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int sp = 0; sp < DA_SPLIT; ++sp) {
      const long idx = ((long)pair * DA_SPLIT + sp) * R + rho;
      const float sw = __builtin_amdgcn_exp2f(part_ml[idx * 2] - m_g);
      l_g += part_ml[idx * 2 + 1] * sw;
      const float* po = part_o + idx * DA_D;
      a0 += po[2 * lane] * sw;
      a1 += po[2 * lane + 1] * sw;
    }
    const float inv = l_g > 0.f ? 1.f / l_g : 0.f;
    *(uint*)(outp + (((long)b * T + tok) * Hq + kvh * REP + g) * DA_D +
             2 * lane) = pack_bf16x2(a0 * inv, a1 * inv);
  }
}

// Phase 2 for every phase-1 kernel of the family (this file's,
// decode_attn_mx.hip's and chunk_attn.hip's): the fp32 partials carry no
// trace of the cache format.  Returns non-zero, launching nothing, unless
// Hq / Hkv is 1, 2, 4 or 8.
extern "C" int decode_attn_merge_launch(const void* part_o,
                                        const void* part_ml, void* outp,
                                        int B, int T, int Hq, int Hkv,
                                        hipStream_t stream) {
  if (B < 1 || T < 1 || Hkv < 1 || Hq % Hkv != 0) return 1;
  return !da_for_rep(Hq / Hkv, [&](auto rep) {
    decode_attn_merge<decltype(rep)::value>
        <<<dim3(B * Hkv, T), 256, 0, stream>>>(
            (const float*)part_o, (const float*)part_ml, (short*)outp, T, Hq,
            Hkv);
  });
}

template <bool RAGGED>
static int da_launch(const void* qlin, const void* klin, const void* vlin,
                     void* kcache, void* vcache, const void* cosp,
                     const void* sinp, const void* pos_ptr, void* part_o,
                     void* part_ml, void* outp, int B, int Hq, int Hkv,
                     int Smax, float scale, int qstride, int kvstride,
                     hipStream_t stream) {
  if (!da_launch_ok(B, Hq, Hkv, Smax, qstride, kvstride)) return 1;
  da_for_rep(Hq / Hkv, [&](auto rep) {
    decode_attn_part<decltype(rep)::value, RAGGED>
        <<<B * Hkv * DA_SPLIT, DA_WAVES * 64, 0, stream>>>(
            (const short*)qlin, (const short*)klin, (const short*)vlin,
            (short*)kcache, (short*)vcache, (const float*)cosp,
            (const float*)sinp, (const long*)pos_ptr, (float*)part_o,
            (float*)part_ml, B, Hq, Hkv, Smax, scale, qstride, kvstride);
  });
  return decode_attn_merge_launch(part_o, part_ml, outp, B, 1, Hq, Hkv,
                                  stream);
}

// Both return non-zero, launching nothing, outside da_launch_ok's contract.
// decode_attn: pos_ptr one int64.  decode_attn_ragged: B of them.
extern "C" int decode_attn(const void* qlin, const void* klin,
                           const void* vlin, void* kcache, void* vcache,
                           const void* cosp, const void* sinp,
                           const void* pos_ptr, void* part_o, void* part_ml,
                           void* outp, int B, int Hq, int Hkv, int Smax,
                           float scale, int qstride, int kvstride,
                           hipStream_t stream) {
  return da_launch<false>(qlin, klin, vlin, kcache, vcache, cosp, sinp,
                          pos_ptr, part_o, part_ml, outp, B, Hq, Hkv, Smax,
                          scale, qstride, kvstride, stream);
}

extern "C" int decode_attn_ragged(const void* qlin, const void* klin,
                                  const void* vlin, void* kcache,
                                  void* vcache, const void* cosp,
                                  const void* sinp, const void* pos_ptr,
                                  void* part_o, void* part_ml, void* outp,
                                  int B, int Hq, int Hkv, int Smax,
                                  float scale, int qstride, int kvstride,
                                  hipStream_t stream) {
  return da_launch<true>(qlin, klin, vlin, kcache, vcache, cosp, sinp,
                         pos_ptr, part_o, part_ml, outp, B, Hq, Hkv, Smax,
                         scale, qstride, kvstride, stream);
}
