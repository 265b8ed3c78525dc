// Fused multi-token ("chunk") decode attention over the paged KV cache for
// CDNA4: T = 2..8 new tokens per sequence, each sequence at its own device
// position, K/V rows in the 16-row pages of a pool behind a block table.  The
// multi-token sibling of paged_decode_attn (paged_attn.hip) and the paged
// sibling of chunk_attn_ragged (chunk_attn.hip): the verify forward of
// per-sequence speculative decoding and chunked prefill on pages.
//
//   paged_chunk_attn    : bf16 pools (PagedKVCache)
//   paged_chunk_attn_mx : MXFP8 pools (PagedMXKVCache: e4m3 payload pages
//                         (num_pages, Hkv, 16, 128) + e8m0 scale pages
//                         (num_pages, Hkv, 16, 4), both uint8); the MX = true
//                         forms of the two kernels below
//
// Token t of sequence b is roped at pos[b] + t, its K/V row goes to slot
// (pos[b] + t) % 16 of page table[b, (pos[b] + t) / 16], and it attends rows
// [0, pos[b] + t] of its sequence as stored.  Three launches on one stream,
// no atomics, no host sync:
//
//   1. paged_chunk_append: block (b, kvh, t).  RoPE of the new K row, then K
//      and V into their page slot, with chunk_attn_append's arithmetic (MX:
//      quantized by mx_quant.h to pack_mx(quantize_mx(row)), eight threads,
//      one per 32-block, into the slot of all four pools).
//   2. paged_chunk_part: workgroup (b, kvh, split), four waves.  The matrix
//      work is chunk_attn_part's: the R = rep * T query rows of a KV head
//      are the N side of 32x32x16 bf16 MFMA tiles (one or two 32-row
//      blocks), the score product is swapped (S^T = K Q^T) so the online
//      softmax is lane-local, P is repacked in registers and O accumulated
//      transposed; each wave stages its own 32-row tile as the dual-use LDS
//      image of mfma.h and the waves merge in LDS at the end.
//   3. decode_attn_merge_launch (decode_attn.hip) over the DA_SPLIT partials.
//
// The page walk.  A 32-row tile is exactly two pages, 2t and 2t + 1 of the
// sequence, in general far apart in the pool.  The staging lane map of
// chunk_attn.hip (step i of 8: row 4i + (lane >> 4), 16-byte chunk lane & 15)
// puts steps 0..3 wholly into the first page and steps 4..7 wholly into the
// second, so the seam falls BETWEEN two load instructions: every load is 16
// bytes, every 16 lanes cover one 256-byte row with four full 64-byte
// requests, and the page of a step is a compile-time choice between two
// wave-uniform page ids.  No lane ever selects a page: the ids live in scalar
// registers and the row address is scalar base + one per-lane offset computed
// once.  The ids of a wave's tile t + 2 * DA_WAVES are fetched (two scalar
// loads) while the rows of tile t + DA_WAVES load into registers and tile t
// is in the MFMAs, so the chain table -> address -> row load never sits
// inside the register prefetch.  The tiles of a sequence are split among the
// DA_SPLIT workgroups by whole tiles, which keeps every split page-aligned,
// and among the four waves round-robin, as in the dense kernel: for the same
// rows the two kernels do the same arithmetic in the same order.
//
// No table entry is trusted.  A sequence is ACTIVE only with 0 <= pos,
// pos + T <= 16 * pages_per_seq and every entry [b, 0 .. (pos + T - 1) / 16]
// inside [0, num_pages) (PagedKVCache.active).  Every workgroup of BOTH
// kernels establishes that with one strided pass over those entries and a
// workgroup vote (pc_active) before its first access to the pools or the
// RoPE table: a chunk whose first page is valid but whose second is not
// writes nothing.  An inactive sequence gets the neutral partial (phase 2
// writes zeros) and nothing else.  Entries beyond page (pos + T - 1) / 16 are
// never read: where the second page of the last tile lies beyond it, its
// steps read the tile's first page instead and are zeroed.  Rows at or beyond
// n = pos + T inside the last tile are ZEROED while staging (a masked P of 0
// times a NaN V would still be NaN in an MFMA, chunk_attn.hip).
//
// MXFP8 pages.  The dequantizing stage of chunk_attn.hip (CaRegs<true>,
// ca_write: e4m3 x e8m0 is exact in bf16) in front of the same LDS image, so
// MFMAs, softmax and merge are the bf16 kernel's own text.  The walk keeps
// its property with the MX staging map (step i of 4: row 8i + (lane >> 3),
// payload bytes 16 (lane & 7) ..+15, the row's four scale bytes as one
// aligned dword): steps 0..1 lie wholly in the first page and steps 2..3 in
// the second, so again the seam falls between two load instructions and the
// page of a step is a compile-time choice between the two scalar ids.  A
// lane keeps two offsets, computed once: (kvh * 16 + (lane >> 3)) * 128 +
// 16 (lane & 7) bytes into a payload page and (kvh * 16 + (lane >> 3)) * 4
// into a scale page; step i adds 8 (i & 1) rows to both.  The eight lanes of
// a row read the same scale dword, which the hardware serves as one request.
// Stale rows (at or beyond n) may hold 0xFF, the NaN encodings of e4m3 and
// e8m0: payload and scale word are zeroed by SELECT (never by a product)
// before mxq_scale or the conversion sees them.  A tile is 32 x 132 bytes
// per operand instead of 32 x 256, in 4 + 4 loads per lane instead of 8.
//
// Resource usage (gfx950, no packed fp32), REP 1 / 2 / 4 / 8 with one query
// block, then REP 8 with two; no instantiation has scratch or spills:
//   bf16: 256 VGPRs, 69 / 70 / 70 / 70 SGPRs, 2 waves per SIMD;
//         256 VGPRs + 232 AGPRs, 50 SGPRs, 1 wave per SIMD
//   MX:   238 VGPRs, 75 / 76 / 76 / 76 SGPRs, 2 waves per SIMD;
//         256 VGPRs + 228 AGPRs, 56 SGPRs, 1 wave per SIMD
// LDS 65792 bytes everywhere.  The bf16 numbers are those of the file before
// it carried the MX forms, and the instruction stream of their tile loop is
// unchanged; the scale pools are the LAST kernel arguments so that the
// kernarg offsets of everything else stay as they were.
//
// Rejected:
//   * a separate paged_chunk_attn_mx.hip: a third copy of the tile loop and
//     the wave merge for a kernel that differs only in how a tile's rows
//     reach the LDS image;
//   * gathering the pages into a dense buffer and running chunk_attn_ragged:
//     what the torch chain does, a second pass over every row per layer and
//     step, and a buffer of max_seq rows per sequence that the pool exists
//     to avoid;
//   * one page (16 rows) per tile: the 32x32x16 MFMA takes 32 K rows on its
//     M side, a 16-row tile would run it half empty and double the softmax
//     steps per row;
//   * a per-lane page id (lane-dependent table loads or a select between the
//     two ids per lane): the table load then feeds a vector address and sits
//     inside the prefetch chain, and 64-bit vector address math replaces a
//     scalar base; the lane map above makes it unnecessary;
//   * the sequence's table row staged in LDS by the workgroup: a wave needs
//     two ids per tile and gets them with two scalar loads from a row that
//     stays in the scalar cache; LDS would add a barrier and up to
//     4 * pages_per_seq bytes beside the 64 KB of images;
//   * splits by pages instead of tiles: a split boundary at an odd page
//     would leave half-empty tiles on both sides of it;
//   * folding the append into phase 1: the splits of a head read the new
//     rows, which another workgroup would be writing.
//
// The tile mathematics and the wave merge repeat chunk_attn_part's text
// instead of sharing it: that kernel is measured and validated as it stands
// and stays untouched; the helpers both need unchanged are in
// chunk_attn_common.h.
//
// Layouts: q (B, T, Hq*128), k/v (B, T, Hkv*128) bf16 pre-RoPE with element
// strides (batch, token) and a dense last dim; k_pages / v_pages bf16
// (num_pages, Hkv, 16, 128) contiguous (MX: as above); block_table int32 (B, pages_per_seq)
// contiguous; cos/sin (>= 16 * pages_per_seq, 64) fp32; pos_ptr B device
// int64; workspace as in chunk_attn.hip.

#include "chunk_attn_common.h"

#define PC_ROWS 16                    // rows of a page (PG_ROWS, paged_attn.hip)
#define PC_THREADS (DA_WAVES * 64)
#define PC_SC (DA_D / 32)             // scale bytes of an MXFP8 row
static_assert(CA_TILE == 2 * PC_ROWS, "a tile is two pages");

// Whether sequence b takes part (file header).  The whole workgroup calls it
// before it touches the pools or the RoPE table; the same answer in every
// thread.  The position bounds the pass over the table, so it comes first.
__device__ __forceinline__ bool pc_active(const long* __restrict__ pos_ptr,
                                          const int* __restrict__ block_table,
                                          int b, int T, int num_pages,
                                          int pages_per_seq, int nthreads) {
  const long pos = pos_ptr[b];
  if (!da_active(pos, T, PC_ROWS * pages_per_seq)) return false;  // uniform
  const int* tab = block_table + (long)b * pages_per_seq;
  const int last = (int)((pos + T - 1) / PC_ROWS);
  int ok = 1;
  for (int j = threadIdx.x; j <= last; j += nthreads)
    ok &= (unsigned)tab[j] < (unsigned)num_pages;
  return __syncthreads_and(ok);
}

// ---------------------------------------------------------------------------
// 1. append: block (b, kvh, t), 128 threads
// ---------------------------------------------------------------------------
template <bool MX>
__global__ void __launch_bounds__(128)
paged_chunk_append(const short* __restrict__ kin, const short* __restrict__ vin,
                   void* __restrict__ kpages, void* __restrict__ vpages,
                   const int* __restrict__ block_table,
                   const float* __restrict__ cosp,
                   const float* __restrict__ sinp,
                   const long* __restrict__ pos_ptr, int T, int Hkv,
                   int num_pages, int pages_per_seq, long kv_bs, long kv_ts,
                   uint8_t* __restrict__ ksc, uint8_t* __restrict__ vsc) {
  const int tok = blockIdx.x % T;
  const int pair = blockIdx.x / T;
  const int kvh = pair % Hkv;
  const int b = pair / Hkv;
  const int tid = threadIdx.x;
  if (!pc_active(pos_ptr, block_table, b, T, num_pages, pages_per_seq, 128))
    return;  // the whole block
  const int row = (int)pos_ptr[b] + tok;  // inside [0, 16 * pages_per_seq)
  const int pg = block_table[(long)b * pages_per_seq + row / PC_ROWS];
  const long src = (long)b * kv_bs + (long)tok * kv_ts + kvh * DA_D;
  const long dst = ((long)pg * Hkv + kvh) * PC_ROWS + row % PC_ROWS;

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
    short* out = (short*)(tid < 64 ? kpages : vpages) + dst * DA_D;
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
    uint8_t* pay = (uint8_t*)(tid < 4 ? kpages : vpages) + dst * DA_D + 32 * blk;
    ((uint4v*)pay)[0] = out[0];
    ((uint4v*)pay)[1] = out[1];
    (tid < 4 ? ksc : vsc)[dst * PC_SC + blk] = (uint8_t)(e + 127);
  }
}

// ---------------------------------------------------------------------------
// 2. phase 1.  The page walk of one wave.
// ---------------------------------------------------------------------------
// The pool pages of the two halves of tile t, wave-uniform and in scalar
// registers; t >= t1 gives page 0 twice, which is never dereferenced.  Both
// entries lie at or below page `last` = (pos + T - 1) / 16, which pc_active
// has range-checked: t < t1 means row 32 t exists, so page 2 t <= last, and a
// second page beyond `last` holds no row and falls back on the first.
struct PcIds { int p0, p1; };

__device__ __forceinline__ PcIds pc_ids(const int* __restrict__ tab, int t,
                                        int t1, int last) {
  PcIds id = {0, 0};
  if (t < t1) {
    id.p0 = __builtin_amdgcn_readfirstlane(tab[2 * t]);
    id.p1 = 2 * t + 1 <= last
                ? __builtin_amdgcn_readfirstlane(tab[2 * t + 1]) : id.p0;
  }
  return id;
}

// What a lane adds to a page id to reach its share of a page, computed once
// per kernel.  bf16: the elements of a page and the lane's element offset
// inside one (head, slot l >> 4, chunk l & 15).  MXFP8: the bytes of a page
// in a payload pool and in a scale pool, and the lane's byte offsets inside
// them (head, slot l >> 3; payload chunk l & 7, the slot's scale dword).
template <bool MX> struct PcLane;
template <> struct PcLane<false> { long page_elems, lane_off; };
template <> struct PcLane<true> { long page_pay, page_sc, pay_off, sc_off; };

__device__ __forceinline__ void pc_lane(PcLane<false>& a, int Hkv, int kvh,
                                        int lane) {
  a.page_elems = (long)Hkv * PC_ROWS * DA_D;
  a.lane_off = ((long)kvh * PC_ROWS + (lane >> 4)) * DA_D + 8 * (lane & 15);
}

__device__ __forceinline__ void pc_lane(PcLane<true>& a, int Hkv, int kvh,
                                        int lane) {
  a.page_pay = (long)Hkv * PC_ROWS * DA_D;
  a.page_sc = (long)Hkv * PC_ROWS * PC_SC;
  a.pay_off = ((long)kvh * PC_ROWS + (lane >> 3)) * DA_D + 16 * (lane & 7);
  a.sc_off = ((long)kvh * PC_ROWS + (lane >> 3)) * PC_SC;
}

// bf16: lane l, step i owns row 4i + (l >> 4) of the tile, 16-byte chunk
// l & 15: steps 0..3 are the first page, steps 4..7 the second.  Rows >= n
// are zeroed; their address stays inside the (valid) page of their step.
__device__ __forceinline__ void pc_load(CaRegs<false>& r,
                                        const void* __restrict__ kpages,
                                        const uint8_t*,
                                        const void* __restrict__ vpages,
                                        const uint8_t*, PcIds id,
                                        const PcLane<false>& a, int row0,
                                        int n, int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool ok = row0 + 4 * i + (lane >> 4) < n;
    const long off = (long)(i < 4 ? id.p0 : id.p1) * a.page_elems +
                     a.lane_off + 4 * (i & 3) * DA_D;
    r.k[i] = ca_sel(ok, *(const uint4v*)((const short*)kpages + off));
    r.v[i] = ca_sel(ok, *(const uint4v*)((const short*)vpages + off));
  }
}

// MXFP8: lane l, step i owns row 8i + (l >> 3) of the tile, payload bytes
// 16 (l & 7) ..+15 and the row's scale dword (ca_write picks the byte of the
// lane's 32-block): steps 0..1 are the first page, steps 2..3 the second,
// slots (l >> 3) and 8 + (l >> 3) of each.  Eight lanes read one scale
// dword: one request, merged by the hardware.  Rows >= n may hold the NaN
// bytes of e4m3 and e8m0: payload AND scale word are zeroed by select before
// anything converts them; their addresses stay inside the (valid) page of
// their step.
__device__ __forceinline__ void pc_load(CaRegs<true>& r,
                                        const void* __restrict__ kpages,
                                        const uint8_t* __restrict__ ksc,
                                        const void* __restrict__ vpages,
                                        const uint8_t* __restrict__ vsc,
                                        PcIds id, const PcLane<true>& a,
                                        int row0, int n, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool ok = row0 + 8 * i + (lane >> 3) < n;
    const long pg = i < 2 ? id.p0 : id.p1;
    const long off = pg * a.page_pay + a.pay_off + 8 * (i & 1) * DA_D;
    const long soff = pg * a.page_sc + a.sc_off + 8 * (i & 1) * PC_SC;
    r.k[i] = ca_sel(ok, *(const uint4v*)((const uint8_t*)kpages + off));
    r.v[i] = ca_sel(ok, *(const uint4v*)((const uint8_t*)vpages + off));
    const unsigned ks = *(const unsigned*)(ksc + soff);
    const unsigned vs = *(const unsigned*)(vsc + soff);
    r.ks[i] = ok ? ks : 0u;
    r.vs[i] = ok ? vs : 0u;
  }
}

// Second launch bound as for chunk_attn_part: two workgroups per CU with one
// query block, one with two.
template <int REP, int NQB, bool MX>
__global__ void __launch_bounds__(PC_THREADS, NQB == 1 ? 2 : 1)
paged_chunk_part(const short* __restrict__ qin,
                 const void* __restrict__ kpages,
                 const void* __restrict__ vpages,
                 const int* __restrict__ block_table,
                 const float* __restrict__ cosp, const float* __restrict__ sinp,
                 const long* __restrict__ pos_ptr, float* __restrict__ part_o,
                 float* __restrict__ part_ml, int T, int Hkv, int num_pages,
                 int pages_per_seq, float scale, long q_bs, long q_ts,
                 const uint8_t* __restrict__ ksc,
                 const uint8_t* __restrict__ vsc) {
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

  if (!pc_active(pos_ptr, block_table, b, T, num_pages, pages_per_seq,
                 PC_THREADS)) {
    da_store_neutral(wg, R, PC_THREADS, part_o, part_ml);
    return;  // the whole workgroup
  }
  const int pos = __builtin_amdgcn_readfirstlane((int)pos_ptr[b]);
  const int n = pos + T;  // rows [0, n) exist, n <= 16 * pages_per_seq
  const int last = (n - 1) / PC_ROWS;
  const int ntiles = (n + CA_TILE - 1) / CA_TILE;
  const int tchunk = (ntiles + DA_SPLIT - 1) / DA_SPLIT;
  const int t0 = s * tchunk;
  const int t1 = min(ntiles, t0 + tchunk);
  const int* tab = block_table + (long)b * pages_per_seq;
  PcLane<MX> la;
  pc_lane(la, Hkv, kvh, lane);

  // ---- Q fragments, RoPE'd once: qf[qb][c] = Q[32qb + col][16c + 8hi + j]
  frag_u qf[NQB][8];
  int lim[NQB];  // last cache row this lane's query row attends; -1: none
#pragma unroll
  for (int qb = 0; qb < NQB; ++qb) {
    const int rho = 32 * qb + col;
    const bool valid = rho < R;
    const int tok = valid ? rho / REP : T - 1;
    const int g = rho % REP;
    lim[qb] = valid ? pos + tok : -1;
    const short* src = qin + (long)b * q_bs + (long)tok * q_ts +
                       (kvh * REP + g) * DA_D + 8 * hi;
    const float* cr = cosp + (long)(pos + tok) * (DA_D / 2) + 8 * hi;
    const float* sr = sinp + (long)(pos + tok) * (DA_D / 2) + 8 * hi;
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
  // the ids of the tile whose rows the loop loads next: one tile ahead
  PcIds ahead = pc_ids(tab, t + DA_WAVES, t1, last);
  if (t < t1) {
    pc_load(regs, kpages, ksc, vpages, vsc, pc_ids(tab, t, t1, last), la,
            CA_TILE * t, n, lane);
    ca_write(regs, kimg, vimg, lane);
  }
  ca_wave_sync();
  for (; t < t1; t += DA_WAVES) {
    const bool more = t + DA_WAVES < t1;
    // lands while the rows of tile t + DA_WAVES load
    const PcIds ahead2 = pc_ids(tab, t + 2 * DA_WAVES, t1, last);
    if (more)
      pc_load(regs, kpages, ksc, vpages, vsc, ahead, la,
              CA_TILE * (t + DA_WAVES), n, lane);
    ahead = ahead2;

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
  for (int i = tid; i < R * (DA_D / 4); i += PC_THREADS) {
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
// q_bs/q_ts, kv_bs/kv_ts: element strides (batch, token) of q and of k = v.
// Returns non-zero, launching nothing, outside ca_launch_ok's contract (with
// Smax = 16 * pages_per_seq), with num_pages < 1 or pages_per_seq < 1, or
// with pools or a table that break the aligned loads: 16 bytes for the bf16
// and the payload pools, 4 for the scale pools (a row's scales are one
// dword).
template <bool MX>
static int pc_launch(const void* q, const void* k, const void* v, void* kpages,
                     void* ksc, void* vpages, void* vsc,
                     const void* block_table, const void* cosp,
                     const void* sinp, const void* pos_ptr, void* part_o,
                     void* part_ml, void* outp, int B, int T, int Hq, int Hkv,
                     int num_pages, int pages_per_seq, float scale, long q_bs,
                     long q_ts, long kv_bs, long kv_ts, hipStream_t stream) {
  if (num_pages < 1 || pages_per_seq < 1 ||
      pages_per_seq > 0x7FFFFFFF / PC_ROWS)
    return 1;
  if (!ca_launch_ok(q, k, v, cosp, sinp, B, T, Hq, Hkv,
                    PC_ROWS * pages_per_seq, q_bs, q_ts, kv_bs, kv_ts))
    return 1;
  if (((uintptr_t)kpages | (uintptr_t)vpages) % 16 ||
      (MX && ((uintptr_t)ksc | (uintptr_t)vsc) % 4) ||
      (uintptr_t)block_table % 4 || (uintptr_t)pos_ptr % 8)
    return 1;
  paged_chunk_append<MX><<<B * Hkv * T, 128, 0, stream>>>(
      (const short*)k, (const short*)v, kpages, vpages,
      (const int*)block_table, (const float*)cosp, (const float*)sinp,
      (const long*)pos_ptr, T, Hkv, num_pages, pages_per_seq, kv_bs, kv_ts,
      (uint8_t*)ksc, (uint8_t*)vsc);
  da_for_rep(Hq / Hkv, [&](auto rep) {
    constexpr int R = decltype(rep)::value;
    // two query blocks: rep 8 only
    auto part = paged_chunk_part<R, 1, MX>;
    if constexpr (R == 8)
      if (R * T > 32) part = paged_chunk_part<R, 2, MX>;
    part<<<B * Hkv * DA_SPLIT, PC_THREADS, 0, stream>>>(
        (const short*)q, kpages, vpages, (const int*)block_table,
        (const float*)cosp, (const float*)sinp, (const long*)pos_ptr,
        (float*)part_o, (float*)part_ml, T, Hkv, num_pages, pages_per_seq,
        scale, q_bs, q_ts, (const uint8_t*)ksc, (const uint8_t*)vsc);
  });
  return decode_attn_merge_launch(part_o, part_ml, outp, B, T, Hq, Hkv,
                                  stream);
}

extern "C" int paged_chunk_attn(const void* q, const void* k, const void* v,
                                void* kpages, void* vpages,
                                const void* block_table, const void* cosp,
                                const void* sinp, const void* pos_ptr,
                                void* part_o, void* part_ml, void* outp,
                                int B, int T, int Hq, int Hkv, int num_pages,
                                int pages_per_seq, float scale, long q_bs,
                                long q_ts, long kv_bs, long kv_ts,
                                hipStream_t stream) {
  return pc_launch<false>(q, k, v, kpages, nullptr, vpages, nullptr,
                          block_table, cosp, sinp, pos_ptr, part_o, part_ml,
                          outp, B, T, Hq, Hkv, num_pages, pages_per_seq, scale,
                          q_bs, q_ts, kv_bs, kv_ts, stream);
}

// The same over MXFP8 pages: kpay / vpay uint8 (num_pages, Hkv, 16, 128), ksc
// / vsc uint8 (num_pages, Hkv, 16, 4).
extern "C" int paged_chunk_attn_mx(const void* q, const void* k,
                                   const void* v, void* kpay, void* ksc,
                                   void* vpay, void* vsc,
                                   const void* block_table, const void* cosp,
                                   const void* sinp, const void* pos_ptr,
                                   void* part_o, void* part_ml, void* outp,
                                   int B, int T, int Hq, int Hkv,
                                   int num_pages, int pages_per_seq,
                                   float scale, long q_bs, long q_ts,
                                   long kv_bs, long kv_ts,
                                   hipStream_t stream) {
  return pc_launch<true>(q, k, v, kpay, ksc, vpay, vsc, block_table, cosp,
                         sinp, pos_ptr, part_o, part_ml, outp, B, T, Hq, Hkv,
                         num_pages, pages_per_seq, scale, q_bs, q_ts, kv_bs,
                         kv_ts, stream);
}
