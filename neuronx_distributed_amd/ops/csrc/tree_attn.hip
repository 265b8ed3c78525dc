// Fused tree-masked decode attention for CDNA4: the verify forward of a
// Medusa candidate tree.  T = 2..16 tree nodes per sequence are appended to a
// dense bf16 KV cache (B, Hkv, Smax, 128) at a device position and attend it
// in one pass.  The tree sibling of chunk_attn.hip, which verifies a chain.
//
// The topology is two device int32 vectors of length T, shared by the batch,
// nodes in breadth-first order (root first, sorted by depth):
//   anc[i]   bit j set iff node j is node i or one of its ancestors
//   depth[i] depth of node i (root 0)
// Node i is roped at position pos + depth[i], its K/V row is stored at cache
// row pos + i, and it attends cache row r iff r < pos, or r < pos + T and bit
// r - pos of anc[i] is set.  depth is clamped to [0, T - 1] and bits of anc
// at or above T are dropped, so any content of the two vectors is memory
// safe: a wrong topology gives wrong numbers, never a stray access.
//
// tree_attn takes one device position for the batch, tree_attn_ragged one per
// sequence.  In BOTH forms a sequence whose T rows do not all lie in
// [0, Smax) is inactive (da_active): no append, a neutral partial, zeros out.
//
//   1. tree_attn_append: block (b, kvh, node), RoPE of K at pos + depth,
//      K and V to cache row pos + node.
//   2. tree_attn_part: workgroup (b, kvh, split), the tile mathematics of
//      chunk_attn_part (chunk_attn_common.h: per-wave dual-use LDS image,
//      register prefetch, swapped score MFMA so a lane owns ONE query row,
//      acc8_to_frag repack, transposed O).  The R = rep * T <= 64 query rows
//      (row rho = node * rep + g) are one or two 32-row MFMA blocks.  A lane
//      keeps its node's ancestor word in a register; the mask is one shift
//      and one select per score, and runs only on tiles that reach past row
//      pos - 1.  The T <= 16 new rows span at most two 32-row tiles, so every
//      other tile runs unmasked.  Rows at or beyond pos + T are zeroed while
//      staging and never loaded.
//   3. decode_attn_merge (decode_attn.hip), unchanged.
//
// tree_kv_commit packs the accepted root path down to consecutive cache
// rows: row pos + d takes what row pos + path[b, d] held.  A destination of
// one step can be the source of another (path 0, 3, 5, 7 writes row pos + 3
// and reads it), so one workgroup per (b, kvh) loads every source row into
// registers, passes a barrier and only then stores.  K was roped at
// pos + depth and a node of depth d lands on row pos + d: no re-rotation.
//
// Layouts: q (B, T, Hq*128), k/v (B, T, Hkv*128) bf16 pre-RoPE with element
// strides (batch, node) and a dense last dim; cos/sin (>= Smax, 64) fp32;
// pos_ptr one device int64 (RAGGED: B of them); anc/depth (T) int32;
// workspace as chunk_attn.hip; path (B, L) int32, dense.

#include "chunk_attn_common.h"

#define TA_TMAX 16  // nodes: the ancestor word is 16 bits
#define TA_RMAX 64  // query rows per KV head: two 32-row blocks

__device__ __forceinline__ int ta_depth(const int* depth, int node, int T) {
  return max(min(depth[node], T - 1), 0);
}

// ---------------------------------------------------------------------------
// 1. append: block (b, kvh, node), 128 threads
// ---------------------------------------------------------------------------
template <bool RAGGED>
__global__ void __launch_bounds__(128)
tree_attn_append(const short* __restrict__ kin, const short* __restrict__ vin,
                 short* __restrict__ kc, short* __restrict__ vc,
                 const float* __restrict__ cosp, const float* __restrict__ sinp,
                 const long* __restrict__ pos_ptr,
                 const int* __restrict__ depth, int T, int Hkv, int Smax,
                 long kv_bs, long kv_ts) {
  const int node = blockIdx.x % T;
  const int pair = blockIdx.x / T;
  const int kvh = pair % Hkv;
  const int b = pair / Hkv;
  const int tid = threadIdx.x;
  const long pos = da_pos<RAGGED>(pos_ptr, b);
  if (!da_active(pos, T, Smax)) return;  // the whole block
  const long src = (long)b * kv_bs + (long)node * kv_ts + kvh * DA_D;
  short* dst = (tid < 64 ? kc : vc) + ((long)pair * Smax + pos + node) * DA_D;
  if (tid < 64) {
    const long p = pos + ta_depth(depth, node, T);  // < pos + T <= Smax
    const float cs = cosp[p * (DA_D / 2) + tid];
    const float sn = sinp[p * (DA_D / 2) + tid];
    float lo, hi;
    da_rope_pair(kin, src, tid, cs, sn, lo, hi);
    dst[tid] = f2bits(lo);
    dst[tid + 64] = f2bits(hi);
  } else {
    const int i = tid - 64;
    dst[i] = vin[src + i];
    dst[i + 64] = vin[src + i + 64];
  }
}

// ---------------------------------------------------------------------------
// 2. phase 1
// ---------------------------------------------------------------------------
// One wave's share of a 32-row tile: lane l, step i owns row 4i + (l >> 4),
// 16-byte chunk l & 15.  Rows >= n read row n - 1 and are zeroed.  row0 < n
// is wave-uniform, so the tile's address is a scalar base and a lane keeps
// one 32-bit offset for the whole walk.
__device__ __forceinline__ void ta_load(CaRegs<false>& r, const short* kc,
                                        const short* vc, long head_row,
                                        int row0, int n, int lane) {
  const short* kt = kc + (head_row + row0) * DA_D;
  const short* vt = vc + (head_row + row0) * DA_D;
  const int last = n - 1 - row0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int lr = 4 * i + (lane >> 4);
    const bool ok = lr <= last;
    const int off = (ok ? lr : last) * DA_D + 8 * (lane & 15);
    r.k[i] = ca_sel(ok, *(const uint4v*)(kt + off));
    r.v[i] = ca_sel(ok, *(const uint4v*)(vt + off));
  }
}

// Second launch bound as in chunk_attn_part: one query block leaves room for
// two workgroups per CU, two query blocks run one.
template <int REP, int NQB, bool RAGGED>
__global__ void __launch_bounds__(DA_WAVES * 64, NQB == 1 ? 2 : 1)
tree_attn_part(const short* __restrict__ qin, const short* __restrict__ kc,
               const short* __restrict__ vc, const float* __restrict__ cosp,
               const float* __restrict__ sinp, const long* __restrict__ pos_ptr,
               const int* __restrict__ anc, const int* __restrict__ depth,
               float* __restrict__ part_o, float* __restrict__ part_ml, int T,
               int Hkv, int Smax, float scale, long q_bs, long q_ts) {
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

  const long lpos = da_pos<RAGGED>(pos_ptr, b);
  if (!da_active(lpos, T, Smax)) {
    da_store_neutral(wg, R, DA_WAVES * 64, part_o, part_ml);
    return;  // the whole workgroup, before any barrier
  }
  const int pos = __builtin_amdgcn_readfirstlane((int)lpos);
  const int n = pos + T;  // rows [0, n) exist, n <= Smax
  const int ntiles = (n + CA_TILE - 1) / CA_TILE;
  const int tchunk = (ntiles + DA_SPLIT - 1) / DA_SPLIT;
  const int t0 = s * tchunk;
  const int t1 = min(ntiles, t0 + tchunk);
  const long head_row = (long)pair * Smax;

  // ---- Q fragments, RoPE'd once at the node's depth:
  //      qf[qb][c] = Q[32qb + col][16c + 8hi + j]
  frag_u qf[NQB][8];
  unsigned word[NQB];  // bit j: this lane's query row sees new row pos + j
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    const int rho = 32 * qb + col;
    const bool valid = rho < R;
    const int node = valid ? rho / REP : T - 1;
    const int g = rho % REP;
    word[qb] = valid ? (unsigned)anc[node] & ((1u << T) - 1u) : 0u;
    const int p = pos + ta_depth(depth, node, T);
    const short* src = qin + (long)b * q_bs + (long)node * q_ts +
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
  CaRegs<false> regs;
  bool more = t0 + wid < t1;
  if (more) {
    ta_load(regs, kc, vc, head_row, CA_TILE * (t0 + wid), n, lane);
    ca_write(regs, kimg, vimg, lane);
    ca_wave_sync();
  }
  for (int t = t0 + wid; more; t += DA_WAVES) {
    more = t + DA_WAVES < t1;
    if (more)
      ta_load(regs, kc, vc, head_row, CA_TILE * (t + DA_WAVES), n, lane);

    frag_u kfr[8], vfr[2][4];
#pragma unroll
    for (int c = 0; c < 8; ++c) kfr[c].u4 = img_row_read(kimg, row_base, c);
#pragma unroll
    for (int c16 = 0; c16 < 2; ++c16)
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
        vfr[c16][nb].u4 = img_tr_read(vimg, tr_base, 16 * c16, 32 * nb);

    const int kv0 = CA_TILE * t;
    const bool need_mask = kv0 + CA_TILE > pos;
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
        // Visibility as a row of bits, bit 32 + j for cache row pos + j: 32
        // ones for the old rows (j < 0), the ancestor word for the new ones,
        // zeros from j = T on (the zeroed rest of the tile).  Shifted right
        // by sh so that bit k stands for this lane's tile row 4 hi + k;
        // need_mask and kv0 < pos + T keep sh in [1, 51].  The funnel shift
        // (v_alignbit_b32) takes sh mod 32.
        const int sh = kv0 + 4 * hi - pos + 32;
        const unsigned vis =
            sh < 32 ? __builtin_amdgcn_alignbit(word[qb], ~0u, sh)
                    : __builtin_amdgcn_alignbit(0u, word[qb], sh);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          sc[r] = (vis >> acc_row(r, 0)) & 1u ? sc[r] : DA_NEG;
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
// 3. commit: workgroup (b, kvh), 256 threads.  Thread (d = tid / 16,
//    ch = tid % 16) moves 16-byte chunk ch of step d, K and V.
// ---------------------------------------------------------------------------
template <bool RAGGED>
__global__ void __launch_bounds__(TA_TMAX * 16)
tree_kv_commit_kernel(short* __restrict__ kc, short* __restrict__ vc,
                      const long* __restrict__ pos_ptr,
                      const int* __restrict__ path, int L, int Hkv, int Smax) {
  const int pair = blockIdx.x;
  const int b = pair / Hkv;
  const int d = threadIdx.x >> 4;
  const int ch = threadIdx.x & 15;
  const long pos = da_pos<RAGGED>(pos_ptr, b);
  const int node = d >= 1 && d < L ? path[(long)b * L + d] : -1;
  // a step moves only between two rows of the cache
  const bool ok = node >= 0 && node < TA_TMAX && pos >= 0 &&
                  pos + max(node, d) < (long)Smax;
  const long head_row = (long)pair * Smax + pos;
  uint4v k, v;
  if (ok) {
    const long off = (head_row + node) * DA_D + 8 * ch;
    k = *(const uint4v*)(kc + off);
    v = *(const uint4v*)(vc + off);
  }
  __syncthreads();  // every source row is in registers
  if (ok) {
    const long off = (head_row + d) * DA_D + 8 * ch;
    *(uint4v*)(kc + off) = k;
    *(uint4v*)(vc + off) = v;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// ca_launch_ok's contract with T in [2, 16] and rep * T <= 64.
static inline bool ta_launch_ok(const void* q, const void* k, const void* v,
                                const void* cosp, const void* sinp, int B,
                                int T, int Hq, int Hkv, int Smax, long q_bs,
                                long q_ts, long kv_bs, long kv_ts) {
  if (T < CA_TMIN || T > TA_TMAX || Smax < T) return false;
  if (q_bs < 0 || kv_bs < 0 || q_ts > 0x7FFFFFFFL || kv_ts > 0x7FFFFFFFL ||
      q_ts < 0 || kv_ts < 0)
    return false;
  if (!da_launch_ok(B, Hq, Hkv, Smax, (int)q_ts, (int)kv_ts)) return false;
  if (Hq / Hkv * T > TA_RMAX) return false;
  if (q_bs % 8 || q_ts % 8) return false;
  if (((uintptr_t)q | (uintptr_t)cosp | (uintptr_t)sinp) % 16) return false;
  if (((uintptr_t)k | (uintptr_t)v) % 2) return false;
  return (long)B * Hkv * T <= 0x7FFFFFFFL && (long)Smax + T < 0x7FFFFFFFL;
}

template <bool RAGGED>
static int ta_launch(const void* q, const void* k, const void* v, void* kc,
                     void* vc, const void* cosp, const void* sinp,
                     const void* pos_ptr, const void* anc, const void* depth,
                     void* part_o, void* part_ml, void* outp, int B, int T,
                     int Hq, int Hkv, int Smax, float scale, long q_bs,
                     long q_ts, long kv_bs, long kv_ts, hipStream_t stream) {
  if (!ta_launch_ok(q, k, v, cosp, sinp, B, T, Hq, Hkv, Smax, q_bs, q_ts,
                    kv_bs, kv_ts))
    return 1;
  if (((uintptr_t)kc | (uintptr_t)vc) % 16 ||
      ((uintptr_t)anc | (uintptr_t)depth) % 4)
    return 1;
  tree_attn_append<RAGGED><<<B * Hkv * T, 128, 0, stream>>>(
      (const short*)k, (const short*)v, (short*)kc, (short*)vc,
      (const float*)cosp, (const float*)sinp, (const long*)pos_ptr,
      (const int*)depth, T, Hkv, Smax, kv_bs, kv_ts);
  da_for_rep(Hq / Hkv, [&](auto rep) {
    constexpr int R = decltype(rep)::value;
    // two query blocks: rep 4 above 8 nodes, rep 8 above 4
    auto part = tree_attn_part<R, 1, RAGGED>;
    if constexpr (R >= 4)
      if (R * T > 32) part = tree_attn_part<R, 2, RAGGED>;
    part<<<B * Hkv * DA_SPLIT, DA_WAVES * 64, 0, stream>>>(
        (const short*)q, (const short*)kc, (const short*)vc,
        (const float*)cosp, (const float*)sinp, (const long*)pos_ptr,
        (const int*)anc, (const int*)depth, (float*)part_o, (float*)part_ml,
        T, Hkv, Smax, scale, q_bs, q_ts);
  });
  return decode_attn_merge_launch(part_o, part_ml, outp, B, T, Hq, Hkv,
                                  stream);
}

// q_bs/q_ts, kv_bs/kv_ts: element strides (batch, node) of q and of k = v.
// Both return non-zero, launching nothing, outside ta_launch_ok's contract.
extern "C" int tree_attn(const void* q, const void* k, const void* v,
                         void* kcache, void* vcache, const void* cosp,
                         const void* sinp, const void* pos_ptr,
                         const void* anc, const void* depth, void* part_o,
                         void* part_ml, void* outp, int B, int T, int Hq,
                         int Hkv, int Smax, float scale, long q_bs, long q_ts,
                         long kv_bs, long kv_ts, hipStream_t stream) {
  return ta_launch<false>(q, k, v, kcache, vcache, cosp, sinp, pos_ptr, anc,
                          depth, part_o, part_ml, outp, B, T, Hq, Hkv, Smax,
                          scale, q_bs, q_ts, kv_bs, kv_ts, stream);
}

// The same with pos_ptr B device int64, one per sequence.
extern "C" int tree_attn_ragged(const void* q, const void* k, const void* v,
                                void* kcache, void* vcache, const void* cosp,
                                const void* sinp, const void* pos_ptr,
                                const void* anc, const void* depth,
                                void* part_o, void* part_ml, void* outp, int B,
                                int T, int Hq, int Hkv, int Smax, float scale,
                                long q_bs, long q_ts, long kv_bs, long kv_ts,
                                hipStream_t stream) {
  return ta_launch<true>(q, k, v, kcache, vcache, cosp, sinp, pos_ptr, anc,
                         depth, part_o, part_ml, outp, B, T, Hq, Hkv, Smax,
                         scale, q_bs, q_ts, kv_bs, kv_ts, stream);
}

// path (B, L) int32, 1 <= L <= 16; ragged != 0: pos_ptr holds B positions.
// Returns non-zero, launching nothing, outside that contract.
extern "C" int tree_kv_commit(void* kcache, void* vcache, const void* pos_ptr,
                              const void* path, int B, int L, int Hkv,
                              int Smax, int ragged, hipStream_t stream) {
  if (B < 1 || Hkv < 1 || Smax < 1 || L < 1 || L > TA_TMAX ||
      (long)B * Hkv > 0x7FFFFFFFL)
    return 1;
  if (((uintptr_t)kcache | (uintptr_t)vcache) % 16 || (uintptr_t)path % 4)
    return 1;
  auto fn = ragged ? tree_kv_commit_kernel<true> : tree_kv_commit_kernel<false>;
  fn<<<B * Hkv, TA_TMAX * 16, 0, stream>>>((short*)kcache, (short*)vcache,
                                           (const long*)pos_ptr,
                                           (const int*)path, L, Hkv, Smax);
  return 0;
}
