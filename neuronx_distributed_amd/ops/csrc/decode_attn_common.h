// What the two phase-1 decode-attention kernels share: decode_attn_part
// (decode_attn.hip, bf16 cache) and decode_attn_mx_part (decode_attn_mx.hip,
// MXFP8 cache).  Each kernel keeps its own walk over the cache, its append of
// the new row and its __shared__ arrays, which the helpers take as arguments.
//
// Mapping: WG (b, kvh, split s) flash-decodes rows [r0, r1) of pos/DA_SPLIT.
// A 16-lane QUARTER-wave owns a row, a lane 8 consecutive dims of it, so
// DA_SLOTS = 4 * DA_WAVES rows are in flight and as many partials (m, l,
// o[REP][128]) reach the LDS merge; split 0 adds the new row as slot
// DA_SLOTS.
//
// Layouts (bf16 unless noted): q_lin (B, Hq*D) row-stride qstride,
// k_lin/v_lin (B, Hkv*D) row-stride kvstride (strided fused-QKV views feed
// directly); cos/sin (>= Smax, D/2) fp32; pos_ptr device int64
// (hipGraph-replayable): one for the whole batch, or with RAGGED one per
// sequence (B of them, dense); workspace part_o (B*Hkv*DA_SPLIT, REP, D)
// fp32 + part_ml (..., 2) fp32 holding (m, l) in the exp2 domain, m = -1e30
// for a split without rows.  D = 128.  No atomics.
//
// RAGGED (the *_ragged entries): sequence b appends at pos_ptr[b] and attends
// its own rows only.  A workgroup serves one b, so its position stays
// workgroup-uniform.  A sequence whose new rows do not all lie in [0, Smax)
// is INACTIVE: its workgroups touch neither the cache nor the RoPE table,
// store the neutral partial (m = -1e30, l = 0, o = 0) and leave before the
// first barrier, and phase 2 writes zeros for it.
#pragma once

#include <type_traits>

#include "common.h"

#define DA_D 128
#define DA_NEG (-1e30f)            // m of a softmax state that holds no row
#define DA_LOG2E 1.4426950408889634f
#define DA_WAVES 4                 // waves per workgroup
#define DA_SPLIT 4                 // KV-range splits per (batch, kv-head)
#define DA_SLOTS (4 * DA_WAVES)    // quarter-wave partials merged per WG

// Phase 2 (decode_attn.hip) for every phase-1 kernel of the family, built for
// the same DA_SPLIT: T tokens per sequence, workspace rows t * rep + g, out
// (B, T, Hq * D) bf16.  Returns non-zero, launching nothing, unless Hq / Hkv
// is 1, 2, 4 or 8.
extern "C" int decode_attn_merge_launch(const void* part_o,
                                        const void* part_ml, void* outp,
                                        int B, int T, int Hq, int Hkv,
                                        hipStream_t stream);

// Host: f(std::integral_constant<int, REP>) for rep = REP in {1, 2, 4, 8};
// false, calling nothing, for any other rep.
template <class F>
static inline bool da_for_rep(int rep, F&& f) {
  switch (rep) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
  }
  return false;
}

// The launch contract of both phase-1 kernels: rep in {1, 2, 4, 8}, positive
// sizes, row strides that hold a row, a grid that fits an int.
static inline bool da_launch_ok(int B, int Hq, int Hkv, int Smax, int qstride,
                                int kvstride) {
  if (B < 1 || Hkv < 1 || Hq < Hkv || Hq % Hkv != 0 || Smax < 1 ||
      qstride < Hq * DA_D || kvstride < Hkv * DA_D)
    return false;
  const int rep = Hq / Hkv;
  if (rep != 1 && rep != 2 && rep != 4 && rep != 8) return false;
  return (long)B * Hkv * DA_SPLIT <= 0x7FFFFFFFL;
}

struct DaCoord {
  int wg, s, kvh, b, qh0;  // workgroup: split, kv head, batch, first q head
  int tid, lane, wid;
  int quarter;             // 0..3: which row of the wave's quad
  int hl;                  // lane within the quarter; dims 8*hl .. 8*hl+7
  long pos, r0, r1;        // append position; this split's rows [r0, r1)
};

// pos_ptr[b * pos_stride], the stride a compile-time 0 (one position) or 1
template <bool RAGGED>
__device__ __forceinline__ long da_pos(const long* pos_ptr, int b) {
  return RAGGED ? pos_ptr[b] : *pos_ptr;
}

// a RAGGED sequence takes part only with all T new rows inside the cache
__device__ __forceinline__ bool da_active(long pos, int T, int Smax) {
  return pos >= 0 && pos + T <= (long)Smax;
}

// The neutral partial of an inactive sequence's workgroup: R workspace rows
// of zeros with (m, l) = (-1e30, 0).  The whole workgroup calls it.
__device__ __forceinline__ void da_store_neutral(int wg, int R, int nthreads,
                                                 float* part_o,
                                                 float* part_ml) {
  const int tid = threadIdx.x;
  for (int i = tid; i < R * DA_D; i += nthreads)
    part_o[(long)wg * R * DA_D + i] = 0.f;
  for (int i = tid; i < R; i += nthreads) {
    part_ml[((long)wg * R + i) * 2 + 0] = DA_NEG;
    part_ml[((long)wg * R + i) * 2 + 1] = 0.f;
  }
}

template <int REP, bool RAGGED = false>
__device__ __forceinline__ void da_coord(DaCoord& c, const long* pos_ptr,
                                            int Hkv) {
  c.wg = blockIdx.x;
  c.s = c.wg % DA_SPLIT;
  const int pair = c.wg / DA_SPLIT;
  c.kvh = pair % Hkv;
  c.b = pair / Hkv;
  c.qh0 = c.kvh * REP;
  c.tid = threadIdx.x;
  c.lane = c.tid & 63;
  c.quarter = c.lane >> 4;
  c.hl = c.lane & 15;
  c.wid = __builtin_amdgcn_readfirstlane(c.tid >> 6);
  c.pos = da_pos<RAGGED>(pos_ptr, c.b);
  const long chunk = (c.pos + DA_SPLIT - 1) / DA_SPLIT;
  c.r0 = (long)c.s * chunk;
  c.r1 = min(c.pos, c.r0 + chunk);
}

// RoPE of dims (t, t + 64) of the 128-wide bf16 row at x + base, t < 64
__device__ __forceinline__ void da_rope_pair(const short* x,
                                             long base, int t, float c,
                                             float sn, float& lo, float& hi) {
  const float x0 = bits2f(x[base + t]);
  const float x1 = bits2f(x[base + t + 64]);
  lo = x0 * c - x1 * sn;
  hi = x1 * c + x0 * sn;
}

// RoPE of the REP q heads of this workgroup into qr; threads t < 64
template <int REP>
__device__ __forceinline__ void da_rope_q(const short* qlin,
                                          int qstride, const DaCoord& c,
                                          float cs, float sn,
                                          float (&qr)[REP][DA_D]) {
#pragma unroll
  for (int g = 0; g < REP; ++g)
    da_rope_pair(qlin, (long)c.b * qstride + (c.qh0 + g) * DA_D, c.tid, cs,
                 sn, qr[g][c.tid], qr[g][c.tid + 64]);
}

// this lane's 8 q dims per head, and an empty running softmax state
template <int REP>
__device__ __forceinline__ void da_init_state(const float (&qr)[REP][DA_D],
                                              int hl, float (&qv)[REP][8],
                                              float (&m_run)[REP],
                                              float (&l_run)[REP],
                                              float (&ov)[REP][8]) {
#pragma unroll
  for (int g = 0; g < REP; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j) qv[g][j] = qr[g][8 * hl + j];
#pragma unroll
  for (int g = 0; g < REP; ++g) {
    m_run[g] = DA_NEG;
    l_run[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ov[g][j] = 0.f;
  }
}

// 4-step xor reduce WITHIN each 16-lane quarter (all 4 rows per op)
template <int N>
__device__ __forceinline__ void da_quarter_reduce(float (&part)[N]) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < N; ++i) part[i] += __shfl_xor(part[i], off, 64);
}

// a quarter-wave's partial into merge slot 4*wid + quarter (each quarter-wave
// is an independent partial covering dims 8*hl .. 8*hl+7)
template <int REP>
__device__ __forceinline__ void da_store_partial(
    const DaCoord& c, const float (&ov)[REP][8], const float (&m_run)[REP],
    const float (&l_run)[REP], float (&merge_o)[DA_SLOTS + 1][REP][DA_D],
    float (&merge_ml)[DA_SLOTS + 1][REP][2]) {
  const int slot = 4 * c.wid + c.quarter;
#pragma unroll
  for (int g = 0; g < REP; ++g) {
#pragma unroll
    for (int j = 0; j < 8; ++j) merge_o[slot][g][8 * c.hl + j] = ov[g][j];
    if (c.hl == 0) {
      merge_ml[slot][g][0] = m_run[g];
      merge_ml[slot][g][1] = l_run[g];
    }
  }
}

// The new row's term into slot DA_SLOTS, from the fp32 LDS rows kn (roped)
// and vn; one wave of split 0 calls it.  All quarters compute the same score;
// each writes its dims.
template <int REP>
__device__ __forceinline__ void da_new_row_term(
    const DaCoord& c, const float (&qv)[REP][8], const float (&kn)[DA_D],
    const float (&vn)[DA_D], float s2,
    float (&merge_o)[DA_SLOTS + 1][REP][DA_D],
    float (&merge_ml)[DA_SLOTS + 1][REP][2]) {
  float part[REP];
#pragma unroll
  for (int g = 0; g < REP; ++g) {
    part[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) part[g] += qv[g][j] * kn[8 * c.hl + j];
  }
  da_quarter_reduce<REP>(part);
#pragma unroll
  for (int g = 0; g < REP; ++g) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      merge_o[DA_SLOTS][g][8 * c.hl + j] = vn[8 * c.hl + j];
    if (c.lane == 0) {
      merge_ml[DA_SLOTS][g][0] = part[g] * s2;
      merge_ml[DA_SLOTS][g][1] = 1.f;
    }
  }
}

// Merge the DA_SLOTS (+1 in split 0) partials of the workgroup and write the
// split's partial to the workspace; wave w takes heads w, w + DA_WAVES, ...,
// a lane 2 dims.  A split without rows (l = 0) stores m = -1e30 so that
// phase 2 weighs it exp2(-1e30 - m) = 0 whatever the others hold.
template <int REP>
__device__ __forceinline__ void da_merge_store(
    const DaCoord& c, const float (&merge_o)[DA_SLOTS + 1][REP][DA_D],
    const float (&merge_ml)[DA_SLOTS + 1][REP][2], float* part_o,
    float* part_ml) {
  const int nslot = DA_SLOTS + (c.s == 0 ? 1 : 0);
  for (int g = c.wid; g < REP; g += DA_WAVES) {
    float m_g = DA_NEG;
    for (int w = 0; w < nslot; ++w) m_g = fmaxf(m_g, merge_ml[w][g][0]);
    float l_g = 0.f, a0 = 0.f, a1 = 0.f;
    for (int w = 0; w < nslot; ++w) {
      float sw = __builtin_amdgcn_exp2f(merge_ml[w][g][0] - m_g);
      l_g += merge_ml[w][g][1] * sw;
      a0 += merge_o[w][g][2 * c.lane] * sw;
      a1 += merge_o[w][g][2 * c.lane + 1] * sw;
    }
    float* po = part_o + ((long)c.wg * REP + g) * DA_D;
    po[2 * c.lane] = a0;
    po[2 * c.lane + 1] = a1;
    if (c.lane == 0) {
      part_ml[((long)c.wg * REP + g) * 2 + 0] = l_g > 0.f ? m_g : DA_NEG;
      part_ml[((long)c.wg * REP + g) * 2 + 1] = l_g;
    }
  }
}
