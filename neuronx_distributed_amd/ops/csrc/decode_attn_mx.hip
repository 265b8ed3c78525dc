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
// Scale byte b in 1..254 is 2^(b-127), built as the float with exponent field
// b; byte 0 (all-zero / negligible block) reads as 0.
//
// Layouts: q_lin (B, Hq*D), k_lin/v_lin (B, Hkv*D) bf16 with row strides;
// cos/sin (>= Smax, D/2) fp32; pos_ptr device int64 (hipGraph-replayable);
// workspace part_o (B*Hkv*SPLIT, REP, D) fp32 + part_ml (..., 2) fp32, the
// format decode_attn_merge reads.  D = 128.  No atomics.

#include "common.h"
#include "mfma.h"
#include "mx_quant.h"

#define DAMX_D 128
#define DAMX_LOG2E 1.4426950408889634f
#define DAMX_WAVES 4   // waves per workgroup
#define DAMX_SPLIT 4   // KV-range splits; decode_attn_merge_launch checks it
#define DAMX_RPW 4     // rows per wave and load: one per 16-lane quarter
#ifndef DAMX_U
#define DAMX_U 2       // rows per quarter-wave per iteration
#endif
#define DAMX_SLOTS (DAMX_RPW * DAMX_WAVES)        // partials merged per WG
#define DAMX_RPI (DAMX_U * DAMX_SLOTS)            // rows per WG-iteration

typedef unsigned int uint2v __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));

// phase 2, decode_attn.hip
extern "C" int decode_attn_merge_launch(const void* part_o,
                                        const void* part_ml, void* outp,
                                        int B, int Hq, int Hkv, int splits,
                                        hipStream_t stream);

// 2^(b-127) for b in 1..254; 0 for b = 0
__device__ __forceinline__ float damx_scale(unsigned b) {
  union { unsigned u; float f; } c;
  c.u = b << 23;
  return c.f;
}

// 8 e4m3 bytes in memory order -> 8 floats
__device__ __forceinline__ void damx_cvt8(uint2v w, float* f) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f2v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f2v hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}

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
  int ab = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) ab = mxq_amax_bits(v[i], ab);
  const int e = mxq_block_exp(ab);
  const float inv = mxq_inv_scale(e);
  const float sc = damx_scale((unsigned)(e + 127));
  uint4v out[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned w0, w1;
    mxq_cvt8(v[i], inv, w0, w1);
    out[i >> 1][2 * (i & 1)] = w0;
    out[i >> 1][2 * (i & 1) + 1] = w1;
    float f[8];
    damx_cvt8(uint2v{w0, w1}, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) deq[32 * blk + 8 * i + j] = f[j] * sc;
  }
  uint4v* dst = (uint4v*)(payload + 32 * blk);
  dst[0] = out[0];
  dst[1] = out[1];
  scales[blk] = (uint8_t)(e + 127);
}

template <int REP>
__global__ void __launch_bounds__(DAMX_WAVES * 64)
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
  const int wg = blockIdx.x;
  const int s = wg % DAMX_SPLIT;
  const int pair = wg / DAMX_SPLIT;
  const int kvh = pair % Hkv;
  const int b = pair / Hkv;
  const int qh0 = kvh * REP;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int quarter = lane >> 4;     // 0..3: which row of the quad
  const int hl = lane & 15;          // lane within quarter; dims 8*hl..8*hl+7
  const int blk = hl >> 2;           // the 32-block those dims lie in
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long pos = *pos_ptr;
  const long chunk = (pos + DAMX_SPLIT - 1) / DAMX_SPLIT;
  const long r0 = (long)s * chunk;
  const long r1 = min(pos, r0 + chunk);

  __shared__ float qr[REP][DAMX_D];
  __shared__ short knb[DAMX_D];      // roped new K row, bf16 bits
  __shared__ short vnb[DAMX_D];      // new V row, bf16 bits
  __shared__ float knd[DAMX_D];      // the new rows as the cache holds them
  __shared__ float vnd[DAMX_D];
  __shared__ float merge_o[DAMX_SLOTS + 1][REP][DAMX_D];
  __shared__ float merge_ml[DAMX_SLOTS + 1][REP][2];

  if (tid < 64) {
    const float c = cosp[pos * (DAMX_D / 2) + tid];
    const float sn = sinp[pos * (DAMX_D / 2) + tid];
#pragma unroll
    for (int g = 0; g < REP; ++g) {
      const long base = (long)b * qstride + (qh0 + g) * DAMX_D;
      float x0 = bits2f(qlin[base + tid]);
      float x1 = bits2f(qlin[base + tid + 64]);
      qr[g][tid] = x0 * c - x1 * sn;
      qr[g][tid + 64] = x1 * c + x0 * sn;
    }
    if (s == 0) {
      const long base = (long)b * kvstride + kvh * DAMX_D;
      float x0 = bits2f(klin[base + tid]);
      float x1 = bits2f(klin[base + tid + 64]);
      knb[tid] = f2bits(x0 * c - x1 * sn);
      knb[tid + 64] = f2bits(x1 * c + x0 * sn);
    }
  } else if (tid < 128 && s == 0) {
    const int i = tid - 64;
    vnb[i] = vlin[(long)b * kvstride + kvh * DAMX_D + i];
    vnb[i + 64] = vlin[(long)b * kvstride + kvh * DAMX_D + i + 64];
  }
  __syncthreads();

  const long head_row = ((long)b * Hkv + kvh) * Smax;
  if (s == 0 && tid < 8) {  // one thread per 32-block: 4 of K, 4 of V
    const long row = head_row + pos;
    if (tid < 4)
      damx_append_block(knb, tid, kpay + row * DAMX_D,
                        ksc + row * (DAMX_D / 32), knd);
    else
      damx_append_block(vnb, tid - 4, vpay + row * DAMX_D,
                        vsc + row * (DAMX_D / 32), vnd);
  }

  const uint8_t* kp_h = kpay + head_row * DAMX_D;
  const uint8_t* vp_h = vpay + head_row * DAMX_D;
  const uint8_t* ks_h = ksc + head_row * (DAMX_D / 32);
  const uint8_t* vs_h = vsc + head_row * (DAMX_D / 32);
  const float s2 = scale * DAMX_LOG2E;
  float qv[REP][8];
#pragma unroll
  for (int g = 0; g < REP; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j) qv[g][j] = qr[g][8 * hl + j];

  float m_run[REP], l_run[REP], ov[REP][8];
#pragma unroll
  for (int g = 0; g < REP; ++g) {
    m_run[g] = -1e30f;
    l_run[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ov[g][j] = 0.f;
  }

  // rows of one iteration: r + u * DAMX_SLOTS, u < DAMX_U, with
  // r = r0 + it * DAMX_RPI + 4 * wid + quarter.  The four scale bytes of a
  // row are one aligned dword; the lane keeps byte `blk`.
  struct Rows {
    uint2v k[DAMX_U], v[DAMX_U];
    unsigned ks[DAMX_U], vs[DAMX_U];
  };
  auto load_rows = [&](long r, Rows& t) {
#pragma unroll
    for (int u = 0; u < DAMX_U; ++u) {
      const long ru = r + u * DAMX_SLOTS;
      t.k[u] = uint2v{0, 0};
      t.v[u] = uint2v{0, 0};
      t.ks[u] = 0;
      t.vs[u] = 0;
      if (ru < r1) {
        t.k[u] = *(const uint2v*)(kp_h + ru * DAMX_D + 8 * hl);
        t.v[u] = *(const uint2v*)(vp_h + ru * DAMX_D + 8 * hl);
        t.ks[u] = *(const unsigned*)(ks_h + ru * (DAMX_D / 32));
        t.vs[u] = *(const unsigned*)(vs_h + ru * (DAMX_D / 32));
      }
    }
  };

  long r = r0 + DAMX_RPW * wid + quarter;
  Rows cur;
  load_rows(r, cur);
  while (r < r1) {
    const long rn = r + DAMX_RPI;
    Rows nxt;
    load_rows(rn, nxt);

    float part[DAMX_U][REP];
    float vf[DAMX_U][8];
#pragma unroll
    for (int u = 0; u < DAMX_U; ++u) {
      float kf[8];
      damx_cvt8(cur.k[u], kf);
      damx_cvt8(cur.v[u], vf[u]);
      const float kscale = damx_scale((cur.ks[u] >> (8 * blk)) & 0xff);
#pragma unroll
      for (int g = 0; g < REP; ++g) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += qv[g][j] * kf[j];
        part[u][g] = acc * kscale;
      }
    }
    // 4-step xor reduce within each 16-lane quarter (4 rows per op)
#pragma unroll
    for (int off = 8; off > 0; off >>= 1)
#pragma unroll
      for (int u = 0; u < DAMX_U; ++u)
#pragma unroll
        for (int g = 0; g < REP; ++g)
          part[u][g] += __shfl_xor(part[u][g], off, 64);
#pragma unroll
    for (int g = 0; g < REP; ++g) {
      // rows past r1 carry zero bytes; they are masked out here
      float sc[DAMX_U];
      float m_new = m_run[g];
#pragma unroll
      for (int u = 0; u < DAMX_U; ++u) {
        sc[u] = part[u][g] * s2;
        if (r + u * DAMX_SLOTS < r1) m_new = fmaxf(m_new, sc[u]);
      }
      const float alpha = __builtin_amdgcn_exp2f(m_run[g] - m_new);
      m_run[g] = m_new;
      l_run[g] *= alpha;
#pragma unroll
      for (int j = 0; j < 8; ++j) ov[g][j] *= alpha;
#pragma unroll
      for (int u = 0; u < DAMX_U; ++u) {
        const float p = (r + u * DAMX_SLOTS < r1)
                            ? __builtin_amdgcn_exp2f(sc[u] - m_new) : 0.f;
        l_run[g] += p;
        const float pv = p * damx_scale((cur.vs[u] >> (8 * blk)) & 0xff);
#pragma unroll
        for (int j = 0; j < 8; ++j) ov[g][j] += pv * vf[u][j];
      }
    }
    r = rn;
    cur = nxt;
  }

  // merge: slot = 4*wid + quarter (each quarter-wave is an independent
  // partial covering dims 8*hl..8*hl+7)
  const int slot = DAMX_RPW * wid + quarter;
#pragma unroll
  for (int g = 0; g < REP; ++g) {
#pragma unroll
    for (int j = 0; j < 8; ++j) merge_o[slot][g][8 * hl + j] = ov[g][j];
    if (hl == 0) {
      merge_ml[slot][g][0] = m_run[g];
      merge_ml[slot][g][1] = l_run[g];
    }
  }
  const int nslot = DAMX_SLOTS + (s == 0 ? 1 : 0);
  __syncthreads();  // knd / vnd of the append are visible from here
  if (s == 0 && wid == 0) {
    float part[REP];
#pragma unroll
    for (int g = 0; g < REP; ++g) {
      part[g] = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) part[g] += qv[g][j] * knd[8 * hl + j];
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1)
#pragma unroll
      for (int g = 0; g < REP; ++g)
        part[g] += __shfl_xor(part[g], off, 64);
    // all quarters computed the same new-row score; each writes its dims
#pragma unroll
    for (int g = 0; g < REP; ++g) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        merge_o[DAMX_SLOTS][g][8 * hl + j] = vnd[8 * hl + j];
      if (lane == 0) {
        merge_ml[DAMX_SLOTS][g][0] = part[g] * s2;
        merge_ml[DAMX_SLOTS][g][1] = 1.f;
      }
    }
  }
  __syncthreads();

  for (int g = wid; g < REP; g += DAMX_WAVES) {
    float m_g = -1e30f;
    for (int w = 0; w < nslot; ++w) m_g = fmaxf(m_g, merge_ml[w][g][0]);
    float l_g = 0.f, a0 = 0.f, a1 = 0.f;
    for (int w = 0; w < nslot; ++w) {
      float sw = __builtin_amdgcn_exp2f(merge_ml[w][g][0] - m_g);
      l_g += merge_ml[w][g][1] * sw;
      a0 += merge_o[w][g][2 * lane] * sw;
      a1 += merge_o[w][g][2 * lane + 1] * sw;
    }
    float* po = part_o + ((long)wg * REP + g) * DAMX_D;
    po[2 * lane] = a0;
    po[2 * lane + 1] = a1;
    if (lane == 0) {
      part_ml[((long)wg * REP + g) * 2 + 0] = l_g > 0.f ? m_g : -1e30f;
      part_ml[((long)wg * REP + g) * 2 + 1] = l_g;
    }
  }
}

// Returns non-zero, launching nothing, outside the contract: rep in
// {1, 2, 4, 8}, positive sizes, row strides that hold a row.
extern "C" int decode_attn_mx(const void* qlin, const void* klin,
                              const void* vlin, void* kpay, void* ksc,
                              void* vpay, void* vsc, const void* cosp,
                              const void* sinp, const void* pos_ptr,
                              void* part_o, void* part_ml, void* outp, int B,
                              int Hq, int Hkv, int Smax, float scale,
                              int qstride, int kvstride, hipStream_t stream) {
  if (B < 1 || Hkv < 1 || Hq < Hkv || Hq % Hkv != 0 || Smax < 1 ||
      qstride < Hq * DAMX_D || kvstride < Hkv * DAMX_D)
    return 1;
  const int rep = Hq / Hkv;
  if (rep != 1 && rep != 2 && rep != 4 && rep != 8) return 1;
  if ((long)B * Hkv * DAMX_SPLIT > 0x7FFFFFFFL) return 1;
  dim3 grid1(B * Hkv * DAMX_SPLIT);
#define LAUNCH(R)                                                          \
  decode_attn_mx_part<R><<<grid1, DAMX_WAVES * 64, 0, stream>>>(           \
      (const short*)qlin, (const short*)klin, (const short*)vlin,          \
      (uint8_t*)kpay, (uint8_t*)ksc, (uint8_t*)vpay, (uint8_t*)vsc,        \
      (const float*)cosp, (const float*)sinp, (const long*)pos_ptr,        \
      (float*)part_o, (float*)part_ml, B, Hq, Hkv, Smax, scale, qstride,   \
      kvstride)
  switch (rep) {
    case 1: LAUNCH(1); break;
    case 2: LAUNCH(2); break;
    case 4: LAUNCH(4); break;
    default: LAUNCH(8); break;
  }
#undef LAUNCH
  return decode_attn_merge_launch(part_o, part_ml, outp, B, Hq, Hkv,
                                  DAMX_SPLIT, stream);
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
  int ab = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) ab = mxq_amax_bits(v[i], ab);
  const int e = mxq_block_exp(ab);
  const float inv = mxq_inv_scale(e);
  uint4v out[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned w0, w1;
    mxq_cvt8(v[i], inv, w0, w1);
    out[i >> 1][2 * (i & 1)] = w0;
    out[i >> 1][2 * (i & 1) + 1] = w1;
  }
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
