// Fused multi-token ("chunk") decode attention for CDNA4: T = 2..8 new
// tokens against a KV cache that already holds rows, from a device position.
// The multi-token sibling of decode_attn.hip / decode_attn_mx.hip, for the
// verify forward of speculative decoding and for chunked prefill.
// chunk_attn / chunk_attn_mx take one device position for the batch;
// chunk_attn_ragged / chunk_attn_mx_ragged take one per sequence (RAGGED of
// decode_attn_common.h: an inactive sequence, one whose T rows do not all fit
// the cache, gets no append, a neutral partial and zeros out).
//
//   chunk_attn    : bf16 cache (B, Hkv, Smax, 128)
//   chunk_attn_mx : MXFP8 cache (MXKVCache: e4m3 payload (B, Hkv, Smax, 128)
//                   + e8m0 scales (B, Hkv, Smax, 4), both uint8)
//
// Token t sits at global position pos + t and attends cache rows
// [0, pos + t].  Three launches on one stream, no atomics, no host sync:
//
//   1. chunk_attn_append: RoPE of the T new K rows, then K and V into the
//      cache (bf16, or quantized with mx_quant.h to pack_mx(quantize_mx(.))).
//      A row with pos + t outside [0, Smax) is not written.  Attention then
//      reads EVERY row, the new ones included, from the cache as stored.
//   2. chunk_attn_part: workgroup (b, kvh, split).  The R = rep * T query
//      rows of a KV head (row rho = t * rep + g) are the N side of
//      32x32x16 bf16 MFMA tiles, one or two 32-row blocks; cache rows stream
//      through in 32-row tiles.  As in flash_attn.hip the score MFMA is
//      swapped (S^T = K Q^T) so a lane owns ONE query row and the online
//      softmax (exp2 domain) is lane-local, P is repacked in registers
//      (acc8_to_frag) and O is accumulated transposed, with V through the
//      transposed read of the LDS image.  The four waves of a workgroup
//      take the tiles of the split round-robin, each with its own (m, l, O);
//      they merge in LDS and write one fp32 partial per split.
//   3. decode_attn_merge (decode_attn.hip): log-sum-exp over the DA_SPLIT
//      partials, bf16 out (B, T, Hq * 128).
//
// Rows at or beyond n = min(pos + T, Smax), and the unfilled part of the last
// tile, are ZEROED while staging (K and V) and their address is clamped to
// row n - 1: a masked P of 0 times a NaN V would still be NaN in an MFMA,
// and nothing outside the cache is ever read.  The causal mask runs only on
// tiles that reach past row pos.
//
// MX form: the e4m3 bytes are dequantized (x e8m0 scale, exact in bf16) while
// staging, so the tile loop is the bf16 one.  The scales run along D, which
// is the contraction dim of Q K^T but NOT of P V (there it is the output
// dim), so the block-scaled MFMA cannot serve both products from one staged
// copy; V would need a second, transposed quantization.  Hence plain bf16
// MFMAs after a dequantizing stage.
//
// Staging: PER WAVE, one K image + one V image of a 32-row tile (2 x 8 KB,
// the dual-use image of mfma.h), single-buffered in LDS with the next tile's
// global loads issued into registers before the MFMAs and written after
// them.  A wave's LDS traffic is in order, so the loop needs no workgroup
// barrier, only compiler fences; waves drift apart freely, which is what
// hides the global latency at 8 waves per CU.  Rejected:
//   * a VALU extension of the quarter-wave decode kernel: rep * T up to 64
//     query vectors per KV head is ~20 flop per cache byte, the whole fp32
//     VALU budget at the cache-read rate;
//   * per-workgroup 64-row tiles behind __syncthreads (flash_attn.hip's
//     scheme): with at most two query row blocks the waves would have to
//     split the tile's rows anyway, and every tile would cost a barrier;
//   * K straight from global as the A fragment: a lane would read 16 bytes
//     at a 256-byte stride (a quarter of each 64-byte request used), and the
//     MX form needs the dequantizing pass through registers regardless;
//   * double-buffered images: 128 KB of LDS per workgroup, one workgroup per
//     CU; the register prefetch gives the same overlap at half the LDS.
//
// Layouts: q (B, T, Hq*128), k/v (B, T, Hkv*128) bf16 pre-RoPE with element
// strides (batch, token) and a dense last dim; cos/sin (>= Smax, 64) fp32;
// pos_ptr one device int64 (RAGGED: B of them); workspace part_o
// (B*Hkv*DA_SPLIT, R, 128) fp32, part_ml (..., R, 2) = (m, l) in the exp2
// domain, m = -1e30 for a split without rows, as in decode_attn_common.h.

#include "decode_attn_common.h"
#include "flash_common.h"
#include "mx_quant.h"

#define CA_TMIN 2
#define CA_TMAX 8
#define CA_TILE 32                          // cache rows per tile
#define CA_IMG_B (CA_TILE * IMG_ROW_B)      // one image: 8192 B
#define CA_WAVE_B (2 * CA_IMG_B)            // K image, then V image
#define CA_LDS_B (DA_WAVES * CA_WAVE_B)     // 65536 B
#define CA_OPAD 132                         // floats per row of the merge tile

// the device position, clamped to [-CA_TMAX, Smax]: outside that range no
// row is written and the set of rows attended does not change any more
template <bool RAGGED>
__device__ __forceinline__ int ca_pos(const long* pos_ptr, int b, int Smax) {
  const long p = da_pos<RAGGED>(pos_ptr, b);
  return (int)max(min(p, (long)Smax), -(long)CA_TMAX);
}

// compiler-level ordering of one wave's LDS writes and reads (the hardware
// keeps a wave's LDS operations in order)
__device__ __forceinline__ void ca_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------
// 1. append: block (b, kvh, t), 128 threads
// ---------------------------------------------------------------------------
template <bool MX, bool RAGGED>
__global__ void __launch_bounds__(128)
chunk_attn_append(const short* __restrict__ kin, const short* __restrict__ vin,
                  void* __restrict__ kc, uint8_t* __restrict__ ksc,
                  void* __restrict__ vc, uint8_t* __restrict__ vsc,
                  const float* __restrict__ cosp,
                  const float* __restrict__ sinp,
                  const long* __restrict__ pos_ptr, int T, int Hkv, int Smax,
                  long kv_bs, long kv_ts) {
  const int tok = blockIdx.x % T;
  const int pair = blockIdx.x / T;
  const int kvh = pair % Hkv;
  const int b = pair / Hkv;
  const int tid = threadIdx.x;
  if (RAGGED && !da_active(da_pos<RAGGED>(pos_ptr, b), T, Smax)) return;
  const int row = ca_pos<RAGGED>(pos_ptr, b, Smax) + tok;
  if (row < 0 || row >= Smax) return;  // the whole block
  const long src = (long)b * kv_bs + (long)tok * kv_ts + kvh * DA_D;
  const long dst = ((long)pair * Smax + row);

  __shared__ __attribute__((aligned(16))) short rows[2][DA_D];  // K, V
  if (tid < 64) {
    const float cs = cosp[(long)row * (DA_D / 2) + tid];
    const float sn = sinp[(long)row * (DA_D / 2) + tid];
    float lo, hi;
    da_rope_pair(kin, src, tid, cs, sn, lo, hi);
    rows[0][tid] = f2bits(lo);
    rows[0][tid + 64] = f2bits(hi);
  } else {
    const int i = tid - 64;
    rows[1][i] = vin[src + i];
    rows[1][i + 64] = vin[src + i + 64];
  }
  __syncthreads();
  if (!MX) {
    short* out = (short*)(tid < 64 ? kc : vc) + dst * DA_D;
    const short* in = rows[tid >> 6];
    const int i = tid & 63;
    *(uint*)(out + 2 * i) = *(const uint*)(in + 2 * i);
  } else if (tid < 8) {  // one thread per 32-block: 4 of K, 4 of V
    const int blk = tid & 3;
    const s8v* in = (const s8v*)(rows[tid >> 2] + 32 * blk);
    s8v v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = in[i];
    uint4v out[2];
    const int e = mxq_block32(v, out);
    uint8_t* pay = (uint8_t*)(tid < 4 ? kc : vc) + dst * DA_D + 32 * blk;
    ((uint4v*)pay)[0] = out[0];
    ((uint4v*)pay)[1] = out[1];
    (tid < 4 ? ksc : vsc)[dst * (DA_D / 32) + blk] = (uint8_t)(e + 127);
  }
}

// ---------------------------------------------------------------------------
// 2. phase 1.  Staging of one 32-row tile by one wave.
// ---------------------------------------------------------------------------
template <bool MX> struct CaRegs;
template <> struct CaRegs<false> { uint4v k[8], v[8]; };
template <> struct CaRegs<true> { uint4v k[4], v[4]; unsigned ks[4], vs[4]; };

__device__ __forceinline__ uint4v ca_sel(bool ok, uint4v x) {
  const uint4v z = {0, 0, 0, 0};
  return ok ? x : z;
}

// bf16: lane l, step i owns row 4i + (l >> 4), 16-byte chunk l & 15.
// Rows >= n read row n - 1 and are zeroed.
__device__ __forceinline__ void ca_load(CaRegs<false>& r, const void* kc,
                                        const uint8_t*, const void* vc,
                                        const uint8_t*, long head_row,
                                        int row0, int n, int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int rr = row0 + 4 * i + (lane >> 4);
    const bool ok = rr < n;
    const long off = (head_row + (ok ? rr : n - 1)) * DA_D + 8 * (lane & 15);
    r.k[i] = ca_sel(ok, *(const uint4v*)((const short*)kc + off));
    r.v[i] = ca_sel(ok, *(const uint4v*)((const short*)vc + off));
  }
}

__device__ __forceinline__ void ca_write(const CaRegs<false>& r, char* kimg,
                                         char* vimg, int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int off = img_off(4 * i + (lane >> 4), lane & 15);
    *(uint4v*)(kimg + off) = r.k[i];
    *(uint4v*)(vimg + off) = r.v[i];
  }
}

// MX: lane l, step i owns row 8i + (l >> 3), payload bytes 16 (l & 7) ..+15,
// which lie in the 32-block (l & 7) >> 1; the row's four scale bytes are one
// aligned dword.
__device__ __forceinline__ void ca_load(CaRegs<true>& r, const void* kc,
                                        const uint8_t* ksc, const void* vc,
                                        const uint8_t* vsc, long head_row,
                                        int row0, int n, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = row0 + 8 * i + (lane >> 3);
    const bool ok = rr < n;
    const long ra = head_row + (ok ? rr : n - 1);
    const long off = ra * DA_D + 16 * (lane & 7);
    r.k[i] = ca_sel(ok, *(const uint4v*)((const uint8_t*)kc + off));
    r.v[i] = ca_sel(ok, *(const uint4v*)((const uint8_t*)vc + off));
    const unsigned ks = *(const unsigned*)(ksc + ra * (DA_D / 32));
    const unsigned vs = *(const unsigned*)(vsc + ra * (DA_D / 32));
    r.ks[i] = ok ? ks : 0u;
    r.vs[i] = ok ? vs : 0u;
  }
}

// 8 e4m3 bytes x scale -> 8 bf16 (exact: 4 significant bits, power-of-2 scale)
__device__ __forceinline__ uint4v ca_deq8(unsigned w0, unsigned w1, float sc) {
  float f[8];
  mxq_dcvt8(uint2v{w0, w1}, f);
  uint4v o;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = pack_bf16x2(f[2 * j] * sc, f[2 * j + 1] * sc);
  return o;
}

__device__ __forceinline__ void ca_write(const CaRegs<true>& r, char* kimg,
                                         char* vimg, int lane) {
  const int pc = lane & 7;
  const int sh = 8 * (pc >> 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 8 * i + (lane >> 3);
    const float ksc = mxq_scale((r.ks[i] >> sh) & 0xff);
    const float vsc = mxq_scale((r.vs[i] >> sh) & 0xff);
    const int o0 = img_off(row, 2 * pc), o1 = img_off(row, 2 * pc + 1);
    *(uint4v*)(kimg + o0) = ca_deq8(r.k[i][0], r.k[i][1], ksc);
    *(uint4v*)(kimg + o1) = ca_deq8(r.k[i][2], r.k[i][3], ksc);
    *(uint4v*)(vimg + o0) = ca_deq8(r.v[i][0], r.v[i][1], vsc);
    *(uint4v*)(vimg + o1) = ca_deq8(r.v[i][2], r.v[i][3], vsc);
  }
}

// RoPE of 8 dims d0..d0+7 (d0 < 64) and their partners d0+64.., rounded to
// bf16 as the MFMA takes them
__device__ __forceinline__ void ca_rope8(uint4v xlo, uint4v xhi,
                                         const float* cs, const float* sn,
                                         uint4v& olo, uint4v& ohi) {
  float lo[8], hi[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = 2 * j + h;
      const float x0 = bits2f((short)(h ? xlo[j] >> 16 : xlo[j] & 0xffff));
      const float x1 = bits2f((short)(h ? xhi[j] >> 16 : xhi[j] & 0xffff));
      lo[e] = x0 * cs[e] - x1 * sn[e];
      hi[e] = x1 * cs[e] + x0 * sn[e];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    olo[j] = pack_bf16x2(lo[2 * j], lo[2 * j + 1]);
    ohi[j] = pack_bf16x2(hi[2 * j], hi[2 * j + 1]);
  }
}

// Second launch bound: HIP's minimum waves per SIMD.  With one query block
// two workgroups share a CU (2 x 64 KB of LDS, 256 registers per lane); two
// query blocks need more registers than that and run one workgroup per CU.
template <int REP, int NQB, bool MX, bool RAGGED>
__global__ void __launch_bounds__(DA_WAVES * 64, NQB == 1 ? 2 : 1)
chunk_attn_part(const short* __restrict__ qin, const void* __restrict__ kc,
                const uint8_t* __restrict__ ksc, const void* __restrict__ vc,
                const uint8_t* __restrict__ vsc,
                const float* __restrict__ cosp, const float* __restrict__ sinp,
                const long* __restrict__ pos_ptr, float* __restrict__ part_o,
                float* __restrict__ part_ml, int T, int Hkv, int Smax,
                float scale, long q_bs, long q_ts) {
  __shared__ __attribute__((aligned(16))) char smem[CA_LDS_B];

  const int wg = blockIdx.x;
  const int s = wg % DA_SPLIT;
  const int pair = wg / DA_SPLIT;
  const int kvh = pair % Hkv;
  const int b = pair / Hkv;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31;  // the query row (within a block) of this lane
  const int hi = lane >> 5;
  const int R = REP * T;

  if (RAGGED && !da_active(da_pos<RAGGED>(pos_ptr, b), T, Smax)) {
    da_store_neutral(wg, R, DA_WAVES * 64, part_o, part_ml);
    return;  // the whole workgroup, before any barrier
  }
  const int pos =
      __builtin_amdgcn_readfirstlane(ca_pos<RAGGED>(pos_ptr, b, Smax));
  const int n = max(min(pos + T, Smax), 0);  // rows [0, n) exist
  const int ntiles = (n + CA_TILE - 1) / CA_TILE;
  const int tchunk = (ntiles + DA_SPLIT - 1) / DA_SPLIT;
  const int t0 = s * tchunk;
  const int t1 = min(ntiles, t0 + tchunk);
  const long head_row = (long)pair * Smax;

  // ---- Q fragments, RoPE'd once: qf[qb][c] = Q[32qb + col][16c + 8hi + j]
  frag_u qf[NQB][8];
  int lim[NQB];  // last cache row this lane's query row attends; -1: none
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    const int rho = 32 * qb + col;
    const bool valid = rho < R;
    const int tok = valid ? rho / REP : T - 1;
    const int g = rho % REP;
    lim[qb] = valid ? min(pos + tok, n - 1) : -1;
    const int p = max(min(pos + tok, Smax - 1), 0);
    const short* src = qin + (long)b * q_bs + (long)tok * q_ts +
                       (kvh * REP + g) * DA_D + 8 * hi;
    const float* cr = cosp + (long)p * (DA_D / 2) + 8 * hi;
    const float* sr = sinp + (long)p * (DA_D / 2) + 8 * hi;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint4v xlo = ca_sel(valid, *(const uint4v*)(src + 16 * c));
      const uint4v xhi = ca_sel(valid, *(const uint4v*)(src + 64 + 16 * c));
      float cs[8], sn[8];
      *(f4v*)&cs[0] = *(const f4v*)(cr + 16 * c);
      *(f4v*)&cs[4] = *(const f4v*)(cr + 16 * c + 4);
      *(f4v*)&sn[0] = *(const f4v*)(sr + 16 * c);
      *(f4v*)&sn[4] = *(const f4v*)(sr + 16 * c + 4);
      ca_rope8(xlo, xhi, cs, sn, qf[qb][c].u4, qf[qb][c + 4].u4);
    }
  }

  f32x16 ot[NQB][4] = {};  // O^T[d = 32nb + acc_row][q = col]
  float m_run[NQB], l_run[NQB];
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    m_run[qb] = DA_NEG;
    l_run[qb] = 0.f;
  }
  const float s2 = scale * DA_LOG2E;

  char* kimg = smem + wid * CA_WAVE_B;
  char* vimg = kimg + CA_IMG_B;
  const int row_base = img_row_base(col, hi);
  const int tr_base = img_tr_base(lane);

  // every branch below is on wave-uniform values (wid, pos and kernel
  // arguments): the transposed reads run with all 64 lanes active
  int t = t0 + wid;
  CaRegs<MX> regs;
  if (t < t1) {
    ca_load(regs, kc, ksc, vc, vsc, head_row, CA_TILE * t, n, lane);
    ca_write(regs, kimg, vimg, lane);
  }
  ca_wave_sync();
  for (; t < t1; t += DA_WAVES) {
    const bool more = t + DA_WAVES < t1;
    if (more)
      ca_load(regs, kc, ksc, vc, vsc, head_row, CA_TILE * (t + DA_WAVES), n,
              lane);

    frag_u kfr[8], vfr[2][4];
#pragma unroll
    for (int c = 0; c < 8; ++c) kfr[c].u4 = img_row_read(kimg, row_base, c);
#pragma unroll
    for (int c16 = 0; c16 < 2; ++c16)
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
        vfr[c16][nb].u4 = img_tr_read(vimg, tr_base, 16 * c16, 32 * nb);

    const int kv0 = CA_TILE * t;
    const bool need_mask = kv0 + CA_TILE > pos + 1;
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
      // S^T[k][q] = sum_d K[k][d] Q^T[d][q]
      f32x16 acc = {};
#pragma unroll
      for (int c = 0; c < 8; ++c)
        acc = mfma_bf16(kfr[c].bf, qf[qb][c].bf, acc);
      float sc[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[r] = acc[r] * s2;
      if (need_mask) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          sc[r] = kv0 + acc_row(r, hi) > lim[qb] ? DA_NEG : sc[r];
      }
      float mt = DA_NEG;
#pragma unroll
      for (int r = 0; r < 16; ++r) mt = fmaxf(mt, sc[r]);
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float m_new = fmaxf(m_run[qb], mt);
      // floor: with every row masked so far exp2(sc - m) must be 0, not 1
      const float m_eff = fmaxf(m_new, -1e28f);
      const float alpha = __builtin_amdgcn_exp2f(m_run[qb] - m_eff);
      m_run[qb] = m_new;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) ot[qb][nb] *= alpha;
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sc[r] = __builtin_amdgcn_exp2f(sc[r] - m_eff);
        psum += sc[r];
      }
      frag_u pf[2];
      pf[0] = acc8_to_frag(sc, 0);
      pf[1] = acc8_to_frag(sc, 8);
      // O^T[d][q] += V^T[d][k] P^T[k][q]
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int c16 = 0; c16 < 2; ++c16)
          ot[qb][nb] = mfma_bf16(vfr[c16][nb].bf, pf[c16].bf, ot[qb][nb]);
      psum += __shfl_xor(psum, 32, 64);
      l_run[qb] = l_run[qb] * alpha + psum;
    }

    ca_wave_sync();
    if (more) ca_write(regs, kimg, vimg, lane);
    ca_wave_sync();
  }

  // ---- merge the four waves in LDS (the staging images are free now) ----
  float* obuf = (float*)smem;                        // [32 NQB][CA_OPAD]
  float* mlm = obuf + 32 * NQB * CA_OPAD;            // [DA_WAVES][32 NQB]
  float* mll = mlm + DA_WAVES * 32 * NQB;
  __syncthreads();
  if (hi == 0) {
#pragma unroll
    for (int qb = 0; qb < NQB; ++qb) {
      mlm[wid * 32 * NQB + 32 * qb + col] = m_run[qb];
      mll[wid * 32 * NQB + 32 * qb + col] = l_run[qb];
    }
  }
  __syncthreads();
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    float M = DA_NEG;
#pragma unroll
    for (int w = 0; w < DA_WAVES; ++w)
      M = fmaxf(M, mlm[w * 32 * NQB + 32 * qb + col]);
    const float sw = __builtin_amdgcn_exp2f(m_run[qb] - M);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) ot[qb][nb] *= sw;
  }
  for (int w = 0; w < DA_WAVES; ++w) {
    if (wid == w) {
#pragma unroll
      for (int qb = 0; qb < NQB; ++qb)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            f4v* dst = (f4v*)(obuf + (32 * qb + col) * CA_OPAD + 32 * nb +
                              8 * rg + 4 * hi);
            f4v x = {ot[qb][nb][4 * rg], ot[qb][nb][4 * rg + 1],
                     ot[qb][nb][4 * rg + 2], ot[qb][nb][4 * rg + 3]};
            if (w > 0) x += *dst;
            *dst = x;
          }
    }
    __syncthreads();
  }
  for (int i = tid; i < R * (DA_D / 4); i += DA_WAVES * 64) {
    const int rho = i >> 5, c4 = i & 31;
    *(f4v*)(part_o + ((long)wg * R + rho) * DA_D + 4 * c4) =
        *(const f4v*)(obuf + rho * CA_OPAD + 4 * c4);
  }
  if (tid < R) {
    float M = DA_NEG;
#pragma unroll
    for (int w = 0; w < DA_WAVES; ++w) M = fmaxf(M, mlm[w * 32 * NQB + tid]);
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < DA_WAVES; ++w)
      L += mll[w * 32 * NQB + tid] *
           __builtin_amdgcn_exp2f(mlm[w * 32 * NQB + tid] - M);
    part_ml[((long)wg * R + tid) * 2 + 0] = L > 0.f ? M : DA_NEG;
    part_ml[((long)wg * R + tid) * 2 + 1] = L;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// The launch contract: da_launch_ok's, T in [2, 8] with Smax >= T, strides
// that hold a row and keep the 16-byte loads aligned.
static bool ca_launch_ok(const void* q, const void* k, const void* v,
                         const void* cosp, const void* sinp, int B, int T,
                         int Hq, int Hkv, int Smax, long q_bs, long q_ts,
                         long kv_bs, long kv_ts) {
  if (T < CA_TMIN || T > CA_TMAX || Smax < T) return false;
  if (q_bs < 0 || kv_bs < 0 || q_ts > 0x7FFFFFFFL || kv_ts > 0x7FFFFFFFL ||
      q_ts < 0 || kv_ts < 0)
    return false;
  if (!da_launch_ok(B, Hq, Hkv, Smax, (int)q_ts, (int)kv_ts)) return false;
  if (q_bs % 8 || q_ts % 8) return false;
  if (((uintptr_t)q | (uintptr_t)cosp | (uintptr_t)sinp) % 16) return false;
  if (((uintptr_t)k | (uintptr_t)v) % 2) return false;
  return (long)B * Hkv * T <= 0x7FFFFFFFL && (long)Smax + T < 0x7FFFFFFFL;
}

template <bool MX, bool RAGGED>
static int ca_launch(const void* q, const void* k, const void* v, void* kc,
                     void* ksc, void* vc, void* vsc, const void* cosp,
                     const void* sinp, const void* pos_ptr, void* part_o,
                     void* part_ml, void* outp, int B, int T, int Hq, int Hkv,
                     int Smax, float scale, long q_bs, long q_ts, long kv_bs,
                     long kv_ts, hipStream_t stream) {
  if (!ca_launch_ok(q, k, v, cosp, sinp, B, T, Hq, Hkv, Smax, q_bs, q_ts,
                    kv_bs, kv_ts))
    return 1;
  if (((uintptr_t)kc | (uintptr_t)vc) % 16 ||
      (MX && ((uintptr_t)ksc | (uintptr_t)vsc) % 4))
    return 1;
  chunk_attn_append<MX, RAGGED><<<B * Hkv * T, 128, 0, stream>>>(
      (const short*)k, (const short*)v, kc, (uint8_t*)ksc, vc, (uint8_t*)vsc,
      (const float*)cosp, (const float*)sinp, (const long*)pos_ptr, T, Hkv,
      Smax, kv_bs, kv_ts);
  da_for_rep(Hq / Hkv, [&](auto rep) {
    constexpr int R = decltype(rep)::value;
    // two query blocks: rep 8 only
    auto part = chunk_attn_part<R, 1, MX, RAGGED>;
    if constexpr (R == 8)
      if (R * T > 32) part = chunk_attn_part<R, 2, MX, RAGGED>;
    part<<<B * Hkv * DA_SPLIT, DA_WAVES * 64, 0, stream>>>(
        (const short*)q, kc, (const uint8_t*)ksc, vc, (const uint8_t*)vsc,
        (const float*)cosp, (const float*)sinp, (const long*)pos_ptr,
        (float*)part_o, (float*)part_ml, T, Hkv, Smax, scale, q_bs, q_ts);
  });
  return decode_attn_merge_launch(part_o, part_ml, outp, B, T, Hq, Hkv,
                                  stream);
}

// q_bs/q_ts, kv_bs/kv_ts: element strides (batch, token) of q and of k = v.
// Both return non-zero, launching nothing, outside ca_launch_ok's contract.
extern "C" int chunk_attn(const void* q, const void* k, const void* v,
                          void* kcache, void* vcache, const void* cosp,
                          const void* sinp, const void* pos_ptr, void* part_o,
                          void* part_ml, void* outp, int B, int T, int Hq,
                          int Hkv, int Smax, float scale, long q_bs, long q_ts,
                          long kv_bs, long kv_ts, hipStream_t stream) {
  return ca_launch<false, false>(q, k, v, kcache, nullptr, vcache, nullptr,
                                 cosp, sinp, pos_ptr, part_o, part_ml, outp, B,
                                 T, Hq, Hkv, Smax, scale, q_bs, q_ts, kv_bs,
                                 kv_ts, stream);
}

extern "C" int chunk_attn_mx(const void* q, const void* k, const void* v,
                             void* kpay, void* ksc, void* vpay, void* vsc,
                             const void* cosp, const void* sinp,
                             const void* pos_ptr, void* part_o, void* part_ml,
                             void* outp, int B, int T, int Hq, int Hkv,
                             int Smax, float scale, long q_bs, long q_ts,
                             long kv_bs, long kv_ts, hipStream_t stream) {
  return ca_launch<true, false>(q, k, v, kpay, ksc, vpay, vsc, cosp, sinp,
                                pos_ptr, part_o, part_ml, outp, B, T, Hq, Hkv,
                                Smax, scale, q_bs, q_ts, kv_bs, kv_ts, stream);
}

// The same two with pos_ptr B device int64, one per sequence.
extern "C" int chunk_attn_ragged(const void* q, const void* k, const void* v,
                                 void* kcache, void* vcache, const void* cosp,
                                 const void* sinp, const void* pos_ptr,
                                 void* part_o, void* part_ml, void* outp,
                                 int B, int T, int Hq, int Hkv, int Smax,
                                 float scale, long q_bs, long q_ts, long kv_bs,
                                 long kv_ts, hipStream_t stream) {
  return ca_launch<false, true>(q, k, v, kcache, nullptr, vcache, nullptr,
                                cosp, sinp, pos_ptr, part_o, part_ml, outp, B,
                                T, Hq, Hkv, Smax, scale, q_bs, q_ts, kv_bs,
                                kv_ts, stream);
}

extern "C" int chunk_attn_mx_ragged(const void* q, const void* k,
                                    const void* v, void* kpay, void* ksc,
                                    void* vpay, void* vsc, const void* cosp,
                                    const void* sinp, const void* pos_ptr,
                                    void* part_o, void* part_ml, void* outp,
                                    int B, int T, int Hq, int Hkv, int Smax,
                                    float scale, long q_bs, long q_ts,
                                    long kv_bs, long kv_ts,
                                    hipStream_t stream) {
  return ca_launch<true, true>(q, k, v, kpay, ksc, vpay, vsc, cosp, sinp,
                               pos_ptr, part_o, part_ml, outp, B, T, Hq, Hkv,
                               Smax, scale, q_bs, q_ts, kv_bs, kv_ts, stream);
}
