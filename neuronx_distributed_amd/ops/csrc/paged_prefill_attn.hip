// Fused chunked-prefill attention over the paged KV cache for CDNA4: T new
// tokens per sequence (any T >= 1, meant for T > 8), each sequence at its own
// device position pos[b] and with its own count n[b] <= T of real tokens, K/V
// rows in the 16-row pages of a pool behind a block table.  The compute-bound
// sibling of paged_chunk_attn.hip (T = 2..8, split for decode): the flash
// forward's tile mathematics on a walk over scattered pages.
//
// Token t < n[b] of sequence b is roped at pos[b] + t, its K/V row goes to
// slot (pos[b] + t) % 16 of page table[b, (pos[b] + t) / 16], and it attends
// rows [0, pos[b] + t] of its sequence as stored.  Tokens t >= n[b] are
// padding: nothing is stored for them and their output rows are zero.  Two
// launches on one stream, no atomics, no host sync:
//
//   1. paged_prefill_append: block (b, kvh, page of the chunk).  RoPE of the
//      new K rows of ONE page with da_rope_pair (paged_chunk_append's
//      arithmetic: the stored rows equal that kernel's bit for bit), then K
//      and V through LDS into their slots with 16-byte stores.  The table
//      entry is read once per block and the activity pass over the table runs
//      once per 16 rows, not once per row.
//   2. paged_prefill_fwd: workgroup (b, kv head, token block), eight waves of
//      32 query rows.  The tile mathematics is flash_fwd_kernel's: swapped
//      S^T = K Q^T on the 32x32x16 bf16 MFMA, lane-local online softmax in
//      the exp2 domain, P repacked with pack_bf16x2 + v_permlane32_swap, O
//      accumulated transposed, K and V staged once per 64-row tile as the
//      dual-use LDS image of mfma.h in two buffers with one barrier per tile.
//
// The rows of a workgroup.  Wave w takes q head kvh * REP + w % REP and the 32
// tokens of sub-block w / REP, so a workgroup covers 256 / REP tokens of ALL
// REP heads of its KV head: every K/V tile it stages, a walk over scattered
// pages, serves the whole GQA group instead of being staged once per q head
// as in flash_fwd_kernel.  The token blocks of a sequence are dispatched
// largest-causal-work first (blockIdx.y reversed), as there.
//
// The page walk.  Tiles are aligned to ABSOLUTE rows: tile j is rows
// [64 j, 64 j + 64), pages 4j .. 4j + 3 of the sequence.  Under the staging
// map of flash_fwd_kernel (thread t owns rows 2 (t >> 4) and 2 (t >> 4) + 1,
// 16-byte chunk t & 15) wave w stages rows 8w .. 8w + 7 of the tile: half of
// page 4j + (w >> 1).  One wave-uniform page id per wave and tile is enough;
// it is fetched with a scalar load from the table row one tile AHEAD of the
// row loads (pp_page), so the chain table -> address -> row load never sits
// inside the register prefetch.  No lane selects a page; every load is 16
// bytes and every 16 lanes cover one 256-byte row.
//
// Q is loaded once per wave and roped in registers: fragment chunks c and
// c + 4 of a lane hold d and d + 64 of the same row, so the rotation is
// lane-local (ca_rope8: fp32 from the cos/sin row pos[b] + t, rounded to bf16
// once).
//
// The diagonal.  A wave's rows sit at absolute positions pos + t0 .. pos + t0
// + 31.  Tiles wholly below its first row run unmasked: all prefix tiles are
// of that kind, the steady state.  Tiles that reach into its row range get
// the per-element mask, tiles above its last real row are skipped by a scalar
// branch, the workgroup's loop ends at the row of its last token < n[b], and
// a wave whose tokens are all padding does no MFMA work.
//
// No table entry is trusted.  A sequence is ACTIVE only with 1 <= n <= T,
// 0 <= pos, pos + n <= 16 * pages_per_seq and every entry
// [b, 0 .. (pos + n - 1) / 16] inside [0, num_pages) (PagedKVCache.active with
// n in place of S).  Every workgroup of BOTH kernels establishes that with one
// strided pass over those entries and a workgroup vote (pp_active, after
// pc_active of paged_chunk_attn.hip) before its first access to the pools or
// the RoPE table.  An inactive sequence, n = 0 included, leaves both pools
// untouched and gets zero output.  Entries beyond page (pos + n - 1) / 16 are
// never read: a wave whose page of the last tile lies beyond it stages zeros.
// Rows at or beyond pos + n inside the last tile are ZEROED while staging (a
// masked P of 0 times a NaN V would still be NaN in an MFMA, chunk_attn.hip).
//
// Epilogue as the flash forward's, through LDS and whole 256-byte rows, into
// out (B, T, Hq*128); padding rows and inactive sequences are written as
// zeros.  No lse: nothing reads it.
//
// Resources (hipcc -O3 --offload-arch=gfx950 without packed fp32,
// -Rpass-analysis=kernel-resource-usage): paged_prefill_fwd, all four REP
// alike, 245 VGPRs, 0 AGPRs, 55-56 SGPRs, no scratch, no spills, 64 KB of
// dynamic LDS + 256 B for the workgroup vote, occupancy 2 waves per SIMD (one
// workgroup per CU, as flash_fwd_kernel); paged_prefill_append 16 VGPRs,
// 8448 B of LDS, occupancy 8.
//
// MXFP8 pages (paged_prefill_attn_mx, the MX = true forms of both kernels).
// The pools are PagedMXKVCache's: e4m3 payload (num_pages, Hkv, 16, 128) and
// biased e8m0 scales (num_pages, Hkv, 16, 4), all uint8.  Everything above
// holds word for word; what differs is how a row reaches its page and how a
// tile's rows reach the LDS image.
//
//   Append.  The new rows of the block's page are roped and copied into LDS
//   as above; then thread t < 128 quantizes 32-block t & 3 of slot
//   (t >> 2) & 15 of K (t < 64) or V with mxq_block32 and writes its 32
//   payload bytes and its scale byte, new rows only: 16 rows x 4 blocks x 2
//   operands.  The bytes are pack_mx(quantize_mx(row)), those that
//   paged_chunk_append<true> and the one-token MX kernel store.
//
//   Staging map.  A tile is 64 x 128 payload bytes per operand, 512 threads x
//   16 bytes: thread t owns row t >> 3, payload bytes 16 (t & 7) ..+15, and
//   the row's four scale bytes as one aligned dword (the eight lanes of a row
//   read the same dword, one request).  Wave w therefore stages rows 8w ..
//   8w + 7, the same half of page 4j + (w >> 1) as in the bf16 map: pp_page,
//   the one scalar id per wave and tile fetched a tile ahead, and "no lane
//   selects a page" stay.  A lane keeps two offsets computed once, one into a
//   payload page and one into a scale page, and carries 2 x 4 + 2 registers
//   between load and LDS write where bf16 carries 16.
//
//   Write.  write_tile dequantizes with ca_deq8 / mxq_scale (e4m3 x e8m0 is
//   exact in bf16) into bf16 chunks 2 (t & 7) and 2 (t & 7) + 1 of its row
//   of the same dual-use image.  It sits where the bf16 write sits, after the
//   tile's MFMA section, where the K and V fragments are dead; from the first
//   img_row_read on the loop is one text for both formats.
//
//   Stale rows (at or beyond pos + n in the last tile) may hold 0xFF, the NaN
//   encodings of e4m3 and e8m0: payload AND scale word are zeroed by SELECT
//   before mxq_scale or the conversion sees them, never by a product
//   (pc_load<true> of paged_chunk_attn.hip).  A wave whose page lies beyond
//   `last` reads page 0 and zeroes it the same way.
//
//   The chunk's own rows are read back as stored: token t attends the MXFP8
//   form of rows pos .. pos + t, as the torch chain does on the dequantized
//   gather() after the paged write.
//
// Resources of the MX forms, measured as above: paged_prefill_fwd 238 VGPRs,
// 0 AGPRs, 62-63 SGPRs, no scratch, no spills, the same LDS and occupancy 2;
// paged_prefill_append 53 VGPRs, 46 SGPRs, 8448 B of LDS, occupancy 8.  The
// bf16 forms keep the numbers above; the scale pools are the LAST kernel
// arguments so that the kernarg offsets of everything else stay.
//
// Rejected for the MX forms:
//   * a separate paged_prefill_attn_mx.hip: a third copy of the tile loop
//     for a kernel that differs only in how a tile's rows reach the image
//     (paged_chunk_attn.hip, for the same reason);
//   * the block-scaled MFMA (v_mfma_scale_f32_32x32x64_f8f6f4): K's scales
//     run along d and would fit the score product, but Q would have to be
//     quantized to fp8, which changes the numerics of every format's
//     prefill; V's scales run along d while the PV product contracts over
//     rows, so they are no block scales of that contraction at all;
//   * gathering the pages into a dense bf16 buffer and running
//     paged_prefill_fwd<false>: the dense copy the pool exists to avoid, and
//     a second pass over every row per layer and chunk.
//
// Layouts: q (B, T, Hq*128), k/v (B, T, Hkv*128) bf16 pre-RoPE with element
// strides (batch, token) and a dense last dim; k_pages / v_pages bf16
// (num_pages, Hkv, 16, 128) contiguous (MX: as above); block_table int32 (B, pages_per_seq)
// contiguous; cos/sin (>= 16 * pages_per_seq, 64) fp32; pos_ptr B device
// int64; len_ptr B device int64 or null (n[b] = T); out contiguous.

#include "chunk_attn_common.h"

#define PP_ROWS 16                 // rows of a page (PG_ROWS, paged_attn.hip)
#define PP_QW 32                   // q rows per wave
#define PP_WAVES 8
#define PP_THREADS (PP_WAVES * 64)
#define PP_KV 64                   // rows of a K/V tile: four pages
#define PP_BUF_B (2 * TILE64_B)    // K image, then V image
#define PP_LDS_B (2 * PP_BUF_B)    // two staging buffers: 65,536 B
#define PP_APPEND_THREADS 256
#define PP_SC (DA_D / 32)          // scale bytes of an MXFP8 row
static_assert(PP_KV == 4 * PP_ROWS, "a tile is four pages");
static_assert(PP_WAVES * 8 == PP_KV, "a wave stages half a page");

// Whether sequence b takes part (file header), its position and its count of
// real tokens.  The whole workgroup calls it before it touches the pools or
// the RoPE table; the same answer in every thread.  The position and the
// count bound the pass over the table, so they come first.
__device__ __forceinline__ bool pp_active(const long* __restrict__ pos_ptr,
                                          const long* __restrict__ len_ptr,
                                          const int* __restrict__ block_table,
                                          int b, int T, int num_pages,
                                          int pages_per_seq, int nthreads,
                                          int& pos_out, int& n_out) {
  const long pos = pos_ptr[b];
  const long n = len_ptr ? len_ptr[b] : (long)T;
  if (n < 1 || n > T || !da_active(pos, (int)n, PP_ROWS * pages_per_seq))
    return false;  // uniform
  pos_out = (int)pos;
  n_out = (int)n;
  const int* tab = block_table + (long)b * pages_per_seq;
  const int last = (int)((pos + n - 1) / PP_ROWS);
  int ok = 1;
  for (int j = threadIdx.x; j <= last; j += nthreads)
    ok &= (unsigned)tab[j] < (unsigned)num_pages;
  return __syncthreads_and(ok);
}

// ---------------------------------------------------------------------------
// 1. append: block (b, kvh, i), the i-th page the chunk touches
// ---------------------------------------------------------------------------
// Thread t: rows of parity t >> 7; of a row, threads u = t & 127 < 64 rope the
// K pair (u, u + 64) and the others copy V elements (u - 64, u).  MX: the
// pools are the uint8 payload pools, ksc / vsc the scale pools; thread
// t < 128 then quantizes 32-block t & 3 of slot (t >> 2) & 15 of K (t < 64)
// or V with mxq_block32 and stores its 32 payload bytes and its scale byte.
template <bool MX>
__global__ void __launch_bounds__(PP_APPEND_THREADS)
paged_prefill_append(const short* __restrict__ kin,
                     const short* __restrict__ vin, short* __restrict__ kpages,
                     short* __restrict__ vpages,
                     const int* __restrict__ block_table,
                     const float* __restrict__ cosp,
                     const float* __restrict__ sinp,
                     const long* __restrict__ pos_ptr,
                     const long* __restrict__ len_ptr, int T, int Hkv,
                     int num_pages, int pages_per_seq, long kv_bs, long kv_ts,
                     uint8_t* __restrict__ ksc, uint8_t* __restrict__ vsc) {
  const int kvh = blockIdx.x;
  const int b = blockIdx.z;
  const int tid = threadIdx.x;
  int pos, n;
  if (!pp_active(pos_ptr, len_ptr, block_table, b, T, num_pages, pages_per_seq,
                 PP_APPEND_THREADS, pos, n))
    return;  // the whole block
  const int page = pos / PP_ROWS + (int)blockIdx.y;  // of the sequence
  if (page > (pos + n - 1) / PP_ROWS) return;        // the whole block
  const int r0 = max(pos, PP_ROWS * page);           // rows [r0, r1) are new
  const int r1 = min(pos + n, PP_ROWS * page + PP_ROWS);
  const int pg = block_table[(long)b * pages_per_seq + page];  // range-checked

  __shared__ __attribute__((aligned(16))) short rows[2][PP_ROWS][DA_D];  // K, V
  const int u = tid & 127;
  for (int row = r0 + (tid >> 7); row < r1; row += 2) {
    const long src = (long)b * kv_bs + (long)(row - pos) * kv_ts + kvh * DA_D;
    const int slot = row % PP_ROWS;
    if (u < 64) {
      const float cs = cosp[(long)row * (DA_D / 2) + u];
      const float sn = sinp[(long)row * (DA_D / 2) + u];
      float lo, hi;
      da_rope_pair(kin, src, u, cs, sn, lo, hi);
      rows[0][slot][u] = f2bits(lo);
      rows[0][slot][u + 64] = f2bits(hi);
    } else {
      rows[1][slot][u - 64] = vin[src + u - 64];
      rows[1][slot][u] = vin[src + u];
    }
  }
  __syncthreads();
  if constexpr (MX) {
    // 2 x 16 rows x 4 blocks of 32 elements: one per thread of the first
    // 128, new rows only; nothing else of the slot's page is touched
    const int opv = tid >> 6, slot = (tid >> 2) & 15, blk = tid & 3;
    const int row = PP_ROWS * page + slot;
    if (tid < 128 && row >= r0 && row < r1) {
      const s8v* in = (const s8v*)&rows[opv][slot][32 * blk];
      s8v x[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) x[i] = in[i];
      uint4v out[2];
      const int e = mxq_block32(x, out);
      const long dst = ((long)pg * Hkv + kvh) * PP_ROWS + slot;  // the row
      uint8_t* pay = (uint8_t*)(opv ? vpages : kpages) + dst * DA_D + 32 * blk;
      ((uint4v*)pay)[0] = out[0];
      ((uint4v*)pay)[1] = out[1];
      (opv ? vsc : ksc)[dst * PP_SC + blk] = (uint8_t)(e + 127);
    }
  } else {
    // 2 x 16 rows x 16 chunks of 16 bytes: two per thread, new rows only
    const long dst = ((long)pg * Hkv + kvh) * PP_ROWS * DA_D;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int slot = tid >> 4, c16 = tid & 15;
      const int row = PP_ROWS * page + slot;
      if (row >= r0 && row < r1)
        *(uint4v*)((i ? vpages : kpages) + dst + slot * DA_D + 8 * c16) =
            *(const uint4v*)&rows[i][slot][8 * c16];
    }
  }
}

// ---------------------------------------------------------------------------
// 2. attention
// ---------------------------------------------------------------------------
// The pool page that wave `wid` stages from in tile t: entry 4t + (wid >> 1),
// wave-uniform and in a scalar register.  An entry beyond `last` =
// (pos + n - 1) / 16 is not read (page 0 stands in; its rows are zeroed).
// Entries at or below `last` were range-checked by pp_active.
__device__ __forceinline__ int pp_page(const int* __restrict__ tab, int t,
                                       int wid, int last) {
  const int j = 4 * t + (wid >> 1);
  return j <= last ? __builtin_amdgcn_readfirstlane(tab[j]) : 0;
}

// Zeros for the output rows of tokens [t0, t1) of the REP heads of kv head
// kvh; the whole workgroup calls it.
template <int REP>
__device__ __forceinline__ void pp_store_zero(short* __restrict__ op, int b,
                                              int T, int Hkv, int kvh, int t0,
                                              int t1) {
  const uint4v z = {0, 0, 0, 0};
  const int per_tok = REP * 16;  // 16-byte chunks of the group's heads
  for (int i = threadIdx.x; i < (t1 - t0) * per_tok; i += PP_THREADS) {
    const int t = t0 + i / per_tok, c = i % per_tok;
    *(uint4v*)(op + ((long)b * T + t) * (Hkv * REP * DA_D) +
               kvh * REP * DA_D + 8 * c) = z;
  }
}

// The second launch bound is HIP's minimum waves per SIMD: 2 is one 8-wave
// workgroup per CU, as for flash_fwd_kernel; the 64 KB of LDS would admit a
// second, the 245 VGPRs of the O^T accumulators and the Q, K and V fragments
// do not.
template <int REP, bool MX>
__global__ void __launch_bounds__(PP_THREADS, 2)
paged_prefill_fwd(const short* __restrict__ qin,
                  const short* __restrict__ kpages,
                  const short* __restrict__ vpages,
                  const int* __restrict__ block_table,
                  const float* __restrict__ cosp,
                  const float* __restrict__ sinp,
                  const long* __restrict__ pos_ptr,
                  const long* __restrict__ len_ptr, short* __restrict__ op,
                  int T, int Hkv, int num_pages, int pages_per_seq,
                  float scale, long q_bs, long q_ts,
                  const uint8_t* __restrict__ ksc,
                  const uint8_t* __restrict__ vsc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TOK = PP_QW * PP_WAVES / REP;  // tokens of a workgroup

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31;  // the query row (within the wave) of this lane
  const int hi = lane >> 5;

  // heads on x, token blocks on y REVERSED: largest causal work first
  const int kvh = blockIdx.x;
  const int tb = (int)(gridDim.y - 1 - blockIdx.y);
  const int b = blockIdx.z;
  const int wg_t0 = tb * TOK;
  const int wg_t1 = min(T, wg_t0 + TOK);

  int pos_v = 0, n_v = 0;
  const bool act = pp_active(pos_ptr, len_ptr, block_table, b, T, num_pages,
                             pages_per_seq, PP_THREADS, pos_v, n_v);
  if (!act || wg_t0 >= n_v) {  // inactive, or a block of padding only
    pp_store_zero<REP>(op, b, T, Hkv, kvh, wg_t0, wg_t1);
    return;  // the whole workgroup
  }
  const int pos = __builtin_amdgcn_readfirstlane(pos_v);
  const int n = __builtin_amdgcn_readfirstlane(n_v);
  const int n_rows = pos + n;  // rows [0, n_rows) exist, <= 16 * pages_per_seq
  const int last = (n_rows - 1) / PP_ROWS;
  const int* tab = block_table + (long)b * pages_per_seq;

  const int h = kvh * REP + wid % REP;           // this wave's q head
  const int tw0 = wg_t0 + PP_QW * (wid / REP);   // its first token
  const bool wave_has_rows = tw0 < n;            // wave-uniform
  const int my_t = tw0 + col;
  const int qw0 = pos + tw0;                     // its first absolute row
  const int my_q = my_t < n ? pos + my_t : -1;   // -1: padding, all masked
  // the rows this wave attends end with its last real token's
  const int my_kv_end = pos + min(n, tw0 + PP_QW);
  const int kv_end = pos + min(n, wg_t0 + TOK);  // the workgroup's
  const int ntiles = (kv_end + PP_KV - 1) / PP_KV;

  // ---- Q fragments, roped once: qf[c] = Q[my_t][16c + 8hi + j] ------------
  frag_u qf[8];
  if (wave_has_rows) {
    const int tok = min(my_t, n - 1);  // padding lanes: a real row, unused
    const short* src = qin + (long)b * q_bs + (long)tok * q_ts + h * DA_D +
                       8 * hi;
    const float* cr = cosp + (long)(pos + tok) * (DA_D / 2) + 8 * hi;
    const float* sr = sinp + (long)(pos + tok) * (DA_D / 2) + 8 * hi;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const uint4v xlo = *(const uint4v*)(src + 16 * c);
      const uint4v xhi = *(const uint4v*)(src + 64 + 16 * c);
      float cs[8], sn[8];
      *(f4v*)&cs[0] = *(const f4v*)(cr + 16 * c);
      *(f4v*)&cs[4] = *(const f4v*)(cr + 16 * c + 4);
      *(f4v*)&sn[0] = *(const f4v*)(sr + 16 * c);
      *(f4v*)&sn[4] = *(const f4v*)(sr + 16 * c + 4);
      ca_rope8(xlo, xhi, cs, sn, qf[c].u4, qf[c + 4].u4);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) qf[c].u4 = uint4v{0, 0, 0, 0};
  }

  f32x16 ot[4] = {};  // O^T[d = 32nb + acc_row][q = col]
  float m_run = DA_NEG;
  float l_run = 0.f;
  const float s2 = scale * DA_LOG2E;

  // ---- staging: thread t owns rows {2 (t >> 4), 2 (t >> 4) + 1} of the
  // tile at 16-byte chunk t & 15; the wave's eight rows are slots
  // 8 (wid & 1) .. + 7 of ONE page.  MX (file header): row t >> 3, payload
  // bytes 16 (t & 7) ..+15 and the row's scale dword; kreg[1] / vreg[1] are
  // unused, lane_off is the byte offset into a payload page and sc_off the
  // one into a scale page.
  const int st_c16 = MX ? tid & 7 : tid & 15;
  const int st_r0 = MX ? tid >> 3 : 2 * (tid >> 4), st_r1 = st_r0 + 1;
  const long page_elems = (long)Hkv * PP_ROWS * DA_D;
  const long page_sc = (long)Hkv * PP_ROWS * PP_SC;
  const long lane_off =
      MX ? ((long)kvh * PP_ROWS + 8 * (wid & 1) + (lane >> 3)) * DA_D +
               16 * st_c16
         : ((long)kvh * PP_ROWS + 8 * (wid & 1) + 2 * (lane >> 4)) * DA_D +
               8 * st_c16;
  const long sc_off =
      ((long)kvh * PP_ROWS + 8 * (wid & 1) + (lane >> 3)) * PP_SC;

  uint4v kreg[2], vreg[2];
  unsigned ksw = 0, vsw = 0;  // MX: the scale dwords of the thread's row
  auto issue_loads = [&](int t, int pg) {
    const long off = (long)pg * page_elems + lane_off;
    const bool ok0 = PP_KV * t + st_r0 < n_rows;
    if constexpr (MX) {
      // stale rows (and page 0 standing in for a page beyond `last`) may
      // hold NaN bytes: payload and scale word are zeroed by select
      const long soff = (long)pg * page_sc + sc_off;
      kreg[0] = ca_sel(ok0, *(const uint4v*)((const uint8_t*)kpages + off));
      vreg[0] = ca_sel(ok0, *(const uint4v*)((const uint8_t*)vpages + off));
      const unsigned ks = *(const unsigned*)(ksc + soff);
      const unsigned vs = *(const unsigned*)(vsc + soff);
      ksw = ok0 ? ks : 0u;
      vsw = ok0 ? vs : 0u;
    } else {
      const bool ok1 = PP_KV * t + st_r1 < n_rows;
      kreg[0] = ca_sel(ok0, *(const uint4v*)(kpages + off));
      kreg[1] = ca_sel(ok1, *(const uint4v*)(kpages + off + DA_D));
      vreg[0] = ca_sel(ok0, *(const uint4v*)(vpages + off));
      vreg[1] = ca_sel(ok1, *(const uint4v*)(vpages + off + DA_D));
    }
  };
  auto write_tile = [&](int buf) {
    char* kimg = smem + buf * PP_BUF_B;
    char* vimg = kimg + TILE64_B;
    if constexpr (MX) {
      // dequantized here, after the tile's MFMA section: bf16 chunks
      // 2 (t & 7) and 2 (t & 7) + 1 of the row, both of 32-block (t & 7) >> 1
      const int sh = 8 * (st_c16 >> 1);
      const float kscale = mxq_scale((ksw >> sh) & 0xff);
      const float vscale = mxq_scale((vsw >> sh) & 0xff);
      const int o0 = img_off(st_r0, 2 * st_c16);
      const int o1 = img_off(st_r0, 2 * st_c16 + 1);
      *(uint4v*)(kimg + o0) = ca_deq8(kreg[0][0], kreg[0][1], kscale);
      *(uint4v*)(kimg + o1) = ca_deq8(kreg[0][2], kreg[0][3], kscale);
      *(uint4v*)(vimg + o0) = ca_deq8(vreg[0][0], vreg[0][1], vscale);
      *(uint4v*)(vimg + o1) = ca_deq8(vreg[0][2], vreg[0][3], vscale);
    } else {
      *(uint4v*)(kimg + img_off(st_r0, st_c16)) = kreg[0];
      *(uint4v*)(kimg + img_off(st_r1, st_c16)) = kreg[1];
      *(uint4v*)(vimg + img_off(st_r0, st_c16)) = vreg[0];
      *(uint4v*)(vimg + img_off(st_r1, st_c16)) = vreg[1];
    }
  };

  const int row_base = img_row_base(col, hi);
  const int tr_base = img_tr_base(lane) + TILE64_B;

  // `ahead`: the page of the tile whose rows the loop loads next
  int ahead = pp_page(tab, 1, wid, last);
  issue_loads(0, pp_page(tab, 0, wid, last));
  write_tile(0);
  __syncthreads();
  // Q must have landed before the loop (flash_fwd_kernel)
#pragma unroll
  for (int c = 0; c < 8; ++c) asm volatile("" : "+v"(qf[c].u4));

  // every branch below is on wave-uniform values: the transposed reads run
  // with all 64 lanes active
  int cur = 0;
  for (int t = 0; t < ntiles; ++t, cur ^= 1) {
    const int kv0 = t * PP_KV;
    // lands while the rows of tile t + 1 load
    const int ahead2 = pp_page(tab, t + 2, wid, last);
    if (t + 1 < ntiles) issue_loads(t + 1, ahead);
    ahead = ahead2;

    if (wave_has_rows && kv0 < my_kv_end) {
      const int rowb = row_base + cur * PP_BUF_B;
      const int trb = tr_base + cur * PP_BUF_B;
      // ---- S^T[k][q] = sum_d K[k][d] Q^T[d][q] ---------------------------
      f32x16 acc[2] = {};
      frag_u kfr[2][8];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int c = 0; c < 8; ++c)
          kfr[kb][c].u4 = img_row_read(smem, rowb + kb * (32 * IMG_ROW_B), c);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int c = 0; c < 8; ++c)
          acc[kb] = mfma_bf16(kfr[kb][c].bf, qf[c].bf, acc[kb]);
      __builtin_amdgcn_s_setprio(0);

      // vfr[c16][nb] = V[16 c16 + 8 hi + j][32 nb + col]: lands under the
      // softmax
      frag_u vfr[4][4];
#pragma unroll
      for (int c16 = 0; c16 < 4; ++c16)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          vfr[c16][nb].u4 = img_tr_read(smem, trb, 16 * c16, 32 * nb);

      float sc[2][16];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[kb][r] = acc[kb][r] * s2;
      // the tile reaches into this wave's row range (rows >= n_rows lie
      // above every real row of the wave, so the same mask covers them)
      if (kv0 + PP_KV > qw0) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            sc[kb][r] = kv0 + 32 * kb + acc_row(r, hi) > my_q ? DA_NEG
                                                              : sc[kb][r];
      }

      float mt = DA_NEG;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, sc[kb][r]);
      mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
      const float m_new = fmaxf(m_run, mt);
      // floor: with every row masked so far exp2(sc - m) must be 0, not 1
      const float m_eff = fmaxf(m_new, -1e28f);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_eff);
      m_run = m_new;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) ot[nb] *= alpha;

      float psum = 0.f;
      frag_u pf[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int kb = s >> 1, r0 = 8 * (s & 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float p = __builtin_amdgcn_exp2f(sc[kb][r0 + j] - m_eff);
          sc[kb][r0 + j] = p;
          psum += p;
        }
        pf[s] = acc8_to_frag(sc[kb], r0);
      }
      // ---- O^T[d][q] += V^T[d][k] P^T[k][q] ------------------------------
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

  // ---- epilogue: normalise, transpose back through LDS (the staging buffers
  // are free after the loop's last barrier), whole 256-byte rows ------------
  if (tw0 >= T) return;  // no row of this wave exists (wave-uniform)
  const float inv_l = l_run > 0.f ? 1.f / l_run : 0.f;
  char* otile = smem + wid * (PP_QW * IMG_ROW_B);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      // d = 32 nb + 8 rg + 4 hi .. + 3: chunk 4 nb + rg, half hi
      const uint w0 = pack_bf16x2(ot[nb][4 * rg + 0] * inv_l,
                                  ot[nb][4 * rg + 1] * inv_l);
      const uint w1 = pack_bf16x2(ot[nb][4 * rg + 2] * inv_l,
                                  ot[nb][4 * rg + 3] * inv_l);
      const uint2 st = {w0, w1};
      *(uint2*)(otile + img_off(col, 4 * nb + rg) + 8 * hi) = st;
    }
  }
  ca_wave_sync();
  const long o_ts = (long)Hkv * REP * DA_D;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int p = lane + i * 64;
    const int row = p >> 4, c16 = p & 15;
    const int tg = tw0 + row;
    if (tg < T) {
      // padding rows are written as zeros, whatever their lanes computed
      const uint4v vv =
          ca_sel(tg < n, *(const uint4v*)(otile + img_off(row, c16)));
      *(uint4v*)(op + ((long)b * T + tg) * o_ts + h * DA_D + c16 * 8) = vv;
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// q_bs/q_ts, kv_bs/kv_ts: element strides (batch, token) of q and of k = v;
// len_ptr may be null (every token is real).  Returns non-zero, launching
// nothing, outside the contract: T < 1, rep not in {1, 2, 4, 8}, sizes or
// strides that do not hold a row or break the aligned loads, num_pages < 1 or
// pages_per_seq < 1, or pools that break the aligned loads: 16 bytes for the
// bf16 and the payload pools, 4 for the scale pools (a row's scales are one
// dword).
template <bool MX>
static int pp_launch(const void* q, const void* k, const void* v, void* kpages,
                     void* ksc, void* vpages, void* vsc,
                     const void* block_table, const void* cosp,
                     const void* sinp, const void* pos_ptr,
                     const void* len_ptr, void* outp, int B, int T, int Hq,
                     int Hkv, int num_pages, int pages_per_seq, float scale,
                     long q_bs, long q_ts, long kv_bs, long kv_ts,
                     hipStream_t stream) {
  if (num_pages < 1 || pages_per_seq < 1 ||
      pages_per_seq > 0x7FFFFFFF / PP_ROWS - 1 || T < 1 ||
      T > 0x7FFFFFFF - PP_ROWS * (pages_per_seq + 1))
    return 1;
  if (q_bs < 0 || kv_bs < 0 || q_ts < 0 || kv_ts < 0 ||
      q_ts > 0x7FFFFFFFL || kv_ts > 0x7FFFFFFFL)
    return 1;
  if (!da_launch_ok(B, Hq, Hkv, PP_ROWS * pages_per_seq, (int)q_ts, (int)kv_ts))
    return 1;
  if (q_bs % 8 || q_ts % 8 || B > 65535) return 1;
  if (((uintptr_t)q | (uintptr_t)cosp | (uintptr_t)sinp | (uintptr_t)kpages |
       (uintptr_t)vpages | (uintptr_t)outp) % 16 ||
      ((uintptr_t)k | (uintptr_t)v) % 2 || (uintptr_t)block_table % 4 ||
      (uintptr_t)pos_ptr % 8 || (uintptr_t)len_ptr % 8)
    return 1;
  if (MX && ((uintptr_t)ksc | (uintptr_t)vsc) % 4) return 1;
  const int rep = Hq / Hkv;
  const int tok = PP_QW * PP_WAVES / rep;
  const long nblk = ((long)T + tok - 1) / tok;
  const long npg = ((long)T + 2 * PP_ROWS - 2) / PP_ROWS;  // pages of a chunk
  if (nblk > 65535 || npg > 65535) return 1;
  paged_prefill_append<MX><<<dim3(Hkv, (unsigned)npg, B), PP_APPEND_THREADS,
                             0, stream>>>(
      (const short*)k, (const short*)v, (short*)kpages, (short*)vpages,
      (const int*)block_table, (const float*)cosp, (const float*)sinp,
      (const long*)pos_ptr, (const long*)len_ptr, T, Hkv, num_pages,
      pages_per_seq, kv_bs, kv_ts, (uint8_t*)ksc, (uint8_t*)vsc);
  da_for_rep(rep, [&](auto r) {
    constexpr int R = decltype(r)::value;
    paged_prefill_fwd<R, MX><<<dim3(Hkv, (unsigned)nblk, B), PP_THREADS,
                               PP_LDS_B, stream>>>(
        (const short*)q, (const short*)kpages, (const short*)vpages,
        (const int*)block_table, (const float*)cosp, (const float*)sinp,
        (const long*)pos_ptr, (const long*)len_ptr, (short*)outp, T, Hkv,
        num_pages, pages_per_seq, scale, q_bs, q_ts, (const uint8_t*)ksc,
        (const uint8_t*)vsc);
  });
  return 0;
}

extern "C" int paged_prefill_attn(const void* q, const void* k, const void* v,
                                  void* kpages, void* vpages,
                                  const void* block_table, const void* cosp,
                                  const void* sinp, const void* pos_ptr,
                                  const void* len_ptr, void* outp, int B, int T,
                                  int Hq, int Hkv, int num_pages,
                                  int pages_per_seq, float scale, long q_bs,
                                  long q_ts, long kv_bs, long kv_ts,
                                  hipStream_t stream) {
  return pp_launch<false>(q, k, v, kpages, nullptr, vpages, nullptr,
                          block_table, cosp, sinp, pos_ptr, len_ptr, outp, B,
                          T, Hq, Hkv, num_pages, pages_per_seq, scale, q_bs,
                          q_ts, kv_bs, kv_ts, stream);
}

// The same over MXFP8 pages: kpay / vpay uint8 (num_pages, Hkv, 16, 128), ksc
// / vsc uint8 (num_pages, Hkv, 16, 4).
extern "C" int paged_prefill_attn_mx(const void* q, const void* k,
                                     const void* v, void* kpay, void* ksc,
                                     void* vpay, void* vsc,
                                     const void* block_table, const void* cosp,
                                     const void* sinp, const void* pos_ptr,
                                     const void* len_ptr, void* outp, int B,
                                     int T, int Hq, int Hkv, int num_pages,
                                     int pages_per_seq, float scale, long q_bs,
                                     long q_ts, long kv_bs, long kv_ts,
                                     hipStream_t stream) {
  return pp_launch<true>(q, k, v, kpay, ksc, vpay, vsc, block_table, cosp,
                         sinp, pos_ptr, len_ptr, outp, B, T, Hq, Hkv,
                         num_pages, pages_per_seq, scale, q_bs, q_ts, kv_bs,
                         kv_ts, stream);
}
