// Fused decode attention over an MXFP8 KV cache for CDNA4, plus the prefill
// store that fills that cache.
//
//   decode_attn_mx : RoPE(q,k) + quantize-and-append of the new K/V row +
//                    flash-decode over the quantized cache, GQA-grouped,
//                    split-KV two-phase (phase 2 is decode_attn.hip's merge)
//   mx_kv_store    : bf16 K, V (B, Hkv, S, D), any strides with a dense last
//                    dim -> payload + scales at cache rows [pos, pos + S)
//
// Cache layout (inference/kv_cache.py MXKVCache == microscaling.pack_mx along
// D): payload uint8 (B, Hkv, Smax, D), one e4m3fn byte per element; scales
// uint8 (B, Hkv, Smax, D/32), biased e8m0.  A D = 128 row is 128 + 4 bytes
// instead of 256.
//
// Phase 1 keeps the quarter-wave row mapping of decode_attn.hip: 16 lanes own
// a row, a lane owns 8 consecutive dims = 8 payload bytes (one b64 load) that
// lie inside ONE 32-block, so the block scale is never applied per element:
// the K scale multiplies the lane's partial dot product once, the V scale
// multiplies p once per row.  Bytes become floats through the hardware
// fp8 -> f32 conversion (v_cvt_pk_f32_fp8, the inverse of mx_quant.h's
// cvt_pk_fp8_f32).  A b64 load carries half the bytes of the bf16 kernel's
// b128, so each quarter-wave handles DAMX_U = 2 rows per iteration from
// independent loads: 8 rows and as many bytes in flight per wave-iteration as
// the bf16 kernel, at the same register footprint (q and o stay 8 dims per
// lane; 8 lanes per row would double both and halve the occupancy at rep 8).
//
// The new row: split 0 ropes k, rounds it to bf16 as the bf16 kernel does,
// quantizes k and v with the mx_quant.h pieces (the stored bytes are
// pack_mx(quantize_mx(row))), and adds the row's attention term from the
// DEQUANTIZED bytes, so the output is a function of the cache contents after
// the append and a later step sees the row this step saw.
//
// Constants, the layouts of q/k/v, the RoPE tables and the workspace, and
// every phase-1 piece but the walk over the cache and the append are in
// decode_attn_common.h, shared with decode_attn.hip.
//
// decode_attn_mx takes one device position for the batch;
// decode_attn_mx_ragged takes one per sequence (decode_attn_common.h, RAGGED).

#include "decode_attn_common.h"
#include "mfma.h"
#include "mx_quant.h"

#ifndef DAMX_U
#define DAMX_U 2       // rows per quarter-wave per iteration
#endif
#define DAMX_RPI (DAMX_U * DA_SLOTS)              // rows per WG-iteration

// One thread quantizes the 32-element block `blk` of a 128-wide bf16 row held
// in LDS, writes payload + scale byte to the cache row and the dequantized
// values back to LDS.
__device__ __forceinline__ void damx_append_block(
    const short* __restrict__ row_bits, int blk, uint8_t* __restrict__ payload,
    uint8_t* __restrict__ scales, float* __restrict__ deq) {
  s8v v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) v[i][j] = row_bits[32 * blk + 8 * i + j];
  uint4v out[2];
  const int e = mxq_block32(v, out);
  const float sc = mxq_scale((unsigned)(e + 127));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float f[8];
    mxq_dcvt8(uint2v{out[i >> 1][2 * (i & 1)], out[i >> 1][2 * (i & 1) + 1]},
              f);
#pragma unroll
    for (int j = 0; j < 8; ++j) deq[32 * blk + 8 * i + j] = f[j] * sc;
  }
  uint4v* dst = (uint4v*)(payload + 32 * blk);
  dst[0] = out[0];
  dst[1] = out[1];
  scales[blk] = (uint8_t)(e + 127);
}

template <int REP, bool RAGGED>
__global__ void __launch_bounds__(DA_WAVES * 64)
decode_attn_mx_part(const short* __restrict__ qlin,
                    const short* __restrict__ klin,
                    const short* __restrict__ vlin,
                    uint8_t* __restrict__ kpay, uint8_t* __restrict__ ksc,
                    uint8_t* __restrict__ vpay, uint8_t* __restrict__ vsc,
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
  const int tid = c.tid, quarter = c.quarter, hl = c.hl;
  const int blk = hl >> 2;           // the 32-block the lane's dims lie in
  const long r1 = c.r1;

  __shared__ float qr[REP][DA_D];
  __shared__ short knb[DA_D];        // roped new K row, bf16 bits
  __shared__ short vnb[DA_D];        // new V row, bf16 bits
  __shared__ float knd[DA_D];        // the new rows as the cache holds them
  __shared__ float vnd[DA_D];
  __shared__ float merge_o[DA_SLOTS + 1][REP][DA_D];
  __shared__ float merge_ml[DA_SLOTS + 1][REP][2];

  // only split 0 ropes the new k and loads v
  if (tid < 64) {
    const float cs = cosp[c.pos * (DA_D / 2) + tid];
    const float sn = sinp[c.pos * (DA_D / 2) + tid];
    da_rope_q<REP>(qlin, qstride, c, cs, sn, qr);
    if (c.s == 0) {
      float lo, hi;
      da_rope_pair(klin, (long)c.b * kvstride + c.kvh * DA_D, tid, cs, sn, lo,
                   hi);
      knb[tid] = f2bits(lo);
      knb[tid + 64] = f2bits(hi);
    }
  } else if (tid < 128 && c.s == 0) {
    const int i = tid - 64;
    vnb[i] = vlin[(long)c.b * kvstride + c.kvh * DA_D + i];
    vnb[i + 64] = vlin[(long)c.b * kvstride + c.kvh * DA_D + i + 64];
  }
  __syncthreads();

  const long head_row = ((long)c.b * Hkv + c.kvh) * Smax;
  if (c.s == 0 && tid < 8) {  // one thread per 32-block: 4 of K, 4 of V
    const long row = head_row + c.pos;
    if (tid < 4)
      damx_append_block(knb, tid, kpay + row * DA_D,
                        ksc + row * (DA_D / 32), knd);
    else
      damx_append_block(vnb, tid - 4, vpay + row * DA_D,
                        vsc + row * (DA_D / 32), vnd);
  }

  const uint8_t* kp_h = kpay + head_row * DA_D;
  const uint8_t* vp_h = vpay + head_row * DA_D;
  const uint8_t* ks_h = ksc + head_row * (DA_D / 32);
  const uint8_t* vs_h = vsc + head_row * (DA_D / 32);
  const float s2 = scale * DA_LOG2E;
  float qv[REP][8], m_run[REP], l_run[REP], ov[REP][8];
  da_init_state<REP>(qr, hl, qv, m_run, l_run, ov);

  // rows of one iteration: r + u * DA_SLOTS, u < DAMX_U, with
  // r = r0 + it * DAMX_RPI + 4 * wid + quarter.  The four scale bytes of a
  // row are one aligned dword; the lane keeps byte `blk`.
  struct Rows {
    uint2v k[DAMX_U], v[DAMX_U];
    unsigned ks[DAMX_U], vs[DAMX_U];
  };
  auto load_rows = [&](long r, Rows& t) {
#pragma unroll
    for (int u = 0; u < DAMX_U; ++u) {
      const long ru = r + u * DA_SLOTS;
      t.k[u] = uint2v{0, 0};
      t.v[u] = uint2v{0, 0};
      t.ks[u] = 0;
      t.vs[u] = 0;
      if (ru < r1) {
        t.k[u] = *(const uint2v*)(kp_h + ru * DA_D + 8 * hl);
        t.v[u] = *(const uint2v*)(vp_h + ru * DA_D + 8 * hl);
        t.ks[u] = *(const unsigned*)(ks_h + ru * (DA_D / 32));
        t.vs[u] = *(const unsigned*)(vs_h + ru * (DA_D / 32));
      }
    }
  };

  long r = c.r0 + 4 * c.wid + quarter;
  Rows cur;
  load_rows(r, cur);
  while (r < r1) {
    const long rn = r + DAMX_RPI;
    Rows nxt;
    load_rows(rn, nxt);

    float part[DAMX_U * REP];   // [u][g]
    float vf[DAMX_U][8];
#pragma unroll
    for (int u = 0; u < DAMX_U; ++u) {
      float kf[8];
      mxq_dcvt8(cur.k[u], kf);
      mxq_dcvt8(cur.v[u], vf[u]);
      const float kscale = mxq_scale((cur.ks[u] >> (8 * blk)) & 0xff);
#pragma unroll
      for (int g = 0; g < REP; ++g) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += qv[g][j] * kf[j];
        part[u * REP + g] = acc * kscale;
      }
    }
    da_quarter_reduce<DAMX_U * REP>(part);
#pragma unroll
    for (int g = 0; g < REP; ++g) {
      // rows past r1 carry zero bytes; they are masked out here
      float sc[DAMX_U];
      float m_new = m_run[g];
#pragma unroll
      for (int u = 0; u < DAMX_U; ++u) {
        sc[u] = part[u * REP + g] * s2;
        if (r + u * DA_SLOTS < r1) m_new = fmaxf(m_new, sc[u]);
      }
      const float alpha = __builtin_amdgcn_exp2f(m_run[g] - m_new);
      m_run[g] = m_new;
      l_run[g] *= alpha;
#pragma unroll
      for (int j = 0; j < 8; ++j) ov[g][j] *= alpha;
#pragma unroll
      for (int u = 0; u < DAMX_U; ++u) {
        const float p = (r + u * DA_SLOTS < r1)
                            ? __builtin_amdgcn_exp2f(sc[u] - m_new) : 0.f;
        l_run[g] += p;
        const float pv = p * mxq_scale((cur.vs[u] >> (8 * blk)) & 0xff);
#pragma unroll
        for (int j = 0; j < 8; ++j) ov[g][j] += pv * vf[u][j];
      }
    }
    r = rn;
    cur = nxt;
  }

  da_store_partial<REP>(c, ov, m_run, l_run, merge_o, merge_ml);
  __syncthreads();  // knd / vnd of the append are visible from here
  if (c.s == 0 && c.wid == 0)
    da_new_row_term<REP>(c, qv, knd, vnd, s2, merge_o, merge_ml);
  __syncthreads();
  da_merge_store<REP>(c, merge_o, merge_ml, part_o, part_ml);
}

template <bool RAGGED>
static int damx_launch(const void* qlin, const void* klin, const void* vlin,
                       void* kpay, void* ksc, void* vpay, void* vsc,
                       const void* cosp, const void* sinp,
                       const void* pos_ptr, void* part_o, void* part_ml,
                       void* outp, int B, int Hq, int Hkv, int Smax,
                       float scale, int qstride, int kvstride,
                       hipStream_t stream) {
  if (!da_launch_ok(B, Hq, Hkv, Smax, qstride, kvstride)) return 1;
  da_for_rep(Hq / Hkv, [&](auto rep) {
    decode_attn_mx_part<decltype(rep)::value, RAGGED>
        <<<B * Hkv * DA_SPLIT, DA_WAVES * 64, 0, stream>>>(
            (const short*)qlin, (const short*)klin, (const short*)vlin,
            (uint8_t*)kpay, (uint8_t*)ksc, (uint8_t*)vpay, (uint8_t*)vsc,
            (const float*)cosp, (const float*)sinp, (const long*)pos_ptr,
            (float*)part_o, (float*)part_ml, B, Hq, Hkv, Smax, scale, qstride,
            kvstride);
  });
  return decode_attn_merge_launch(part_o, part_ml, outp, B, 1, Hq, Hkv,
                                  stream);
}

// Both return non-zero, launching nothing, outside da_launch_ok's contract.
// decode_attn_mx: pos_ptr one int64.  decode_attn_mx_ragged: B of them.
extern "C" int decode_attn_mx(const void* qlin, const void* klin,
                              const void* vlin, void* kpay, void* ksc,
                              void* vpay, void* vsc, const void* cosp,
                              const void* sinp, const void* pos_ptr,
                              void* part_o, void* part_ml, void* outp, int B,
                              int Hq, int Hkv, int Smax, float scale,
                              int qstride, int kvstride, hipStream_t stream) {
  return damx_launch<false>(qlin, klin, vlin, kpay, ksc, vpay, vsc, cosp,
                            sinp, pos_ptr, part_o, part_ml, outp, B, Hq, Hkv,
                            Smax, scale, qstride, kvstride, stream);
}

extern "C" int decode_attn_mx_ragged(const void* qlin, const void* klin,
                                     const void* vlin, void* kpay, void* ksc,
                                     void* vpay, void* vsc, const void* cosp,
                                     const void* sinp, const void* pos_ptr,
                                     void* part_o, void* part_ml, void* outp,
                                     int B, int Hq, int Hkv, int Smax,
                                     float scale, int qstride, int kvstride,
                                     hipStream_t stream) {
  return damx_launch<true>(qlin, klin, vlin, kpay, ksc, vpay, vsc, cosp,
                           sinp, pos_ptr, part_o, part_ml, outp, B, Hq, Hkv,
                           Smax, scale, qstride, kvstride, stream);
}

// ---------------------------------------------------------------------------
// mx_kv_store: one thread per 32-element block of K and of V.
// Strides are in elements: (batch, head, seq); the last dim is dense.
// ---------------------------------------------------------------------------
struct MxKvSrc {
  const short* p;
  long sb, sh, ss;
};

extern "C" __global__ void __launch_bounds__(256)
mx_kv_store_kernel(MxKvSrc ksrc, MxKvSrc vsrc, uint8_t* __restrict__ kpay,
                   uint8_t* __restrict__ ksc, uint8_t* __restrict__ vpay,
                   uint8_t* __restrict__ vsc, int B, int H, int S, int D,
                   int Smax, long pos) {
  const int bpr = D / 32;
  const long per = (long)B * H * S * bpr;  // blocks of one operand
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * per) return;
  const bool is_v = idx >= per;
  if (is_v) idx -= per;
  const int kb = (int)(idx % bpr);
  long t = idx / bpr;
  const int sq = (int)(t % S);
  t /= S;
  const int h = (int)(t % H);
  const int b = (int)(t / H);
  const MxKvSrc src = is_v ? vsrc : ksrc;
  uint8_t* pay = is_v ? vpay : kpay;
  uint8_t* scl = is_v ? vsc : ksc;

  const s8v* in =
      (const s8v*)(src.p + b * src.sb + h * src.sh + sq * src.ss + 32 * kb);
  s8v v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = in[i];
  uint4v out[2];
  const int e = mxq_block32(v, out);
  const long row = ((long)b * H + h) * Smax + pos + sq;
  uint4v* dst = (uint4v*)(pay + row * D + 32 * kb);
  dst[0] = out[0];
  dst[1] = out[1];
  scl[row * bpr + kb] = (uint8_t)(e + 127);
}

// kstr / vstr: the four element strides (batch, head, seq, last) of k and v.
// Returns non-zero, launching nothing, on a contract violation: rows past
// the cache (pos + S > Smax), D % 32 != 0, a non-dense last dim, or strides
// that break the 16-byte loads.
extern "C" int mx_kv_store(const void* k, const void* v, const long* kstr,
                           const long* vstr, void* kpay, void* ksc,
                           void* vpay, void* vsc, int B, int H, int S, int D,
                           int Smax, long pos, hipStream_t stream) {
  if (B < 1 || H < 1 || S < 1 || D < 32 || D % 32 != 0 || Smax < 1) return 1;
  if (pos < 0 || pos + S > Smax) return 1;
  if (kstr[3] != 1 || vstr[3] != 1) return 1;
  for (int i = 0; i < 3; ++i)
    if (kstr[i] < 0 || vstr[i] < 0 || kstr[i] % 8 != 0 || vstr[i] % 8 != 0)
      return 1;
  if (((uintptr_t)k | (uintptr_t)v | (uintptr_t)kpay | (uintptr_t)vpay) % 16)
    return 1;
  const long nblk = 2L * B * H * S * (D / 32);
  const long grid = (nblk + 255) / 256;
  if (grid > 0x7FFFFFFFL) return 1;
  const MxKvSrc ks = {(const short*)k, kstr[0], kstr[1], kstr[2]};
  const MxKvSrc vs = {(const short*)v, vstr[0], vstr[1], vstr[2]};
  mx_kv_store_kernel<<<(unsigned)grid, 256, 0, stream>>>(
      ks, vs, (uint8_t*)kpay, (uint8_t*)ksc, (uint8_t*)vpay, (uint8_t*)vsc, B,
      H, S, D, Smax, pos);
  return 0;
}
