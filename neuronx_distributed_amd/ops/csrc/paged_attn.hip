// Paged KV cache for CDNA4: fused one-token decode attention that walks the
// pages of each sequence through a block table, and the prefill store into
// the pages.
//
//   paged_decode_attn : RoPE(q,k) + append into the sequence's page +
//                       flash-decode over its pages, GQA-grouped, split-KV;
//                       phase 2 is decode_attn_merge_launch (decode_attn.hip)
//   paged_kv_store    : bf16 K, V (B, Hkv, S, D), any strides with a dense
//                       last dim, into the pages of rows [pos0, pos0 + S)
//
// Layouts: k_pages / v_pages bf16 (num_pages, Hkv, PG_ROWS, 128), contiguous;
// block_table int32 (B, pages_per_seq), contiguous: entry [b, j] is the pool
// page of rows [16 j, 16 j + 16) of sequence b, -1 = not allocated; pos_ptr
// one device int64 per sequence.  Everything else as in decode_attn_common.h.
//
// PG_ROWS = DA_SLOTS: the workgroup's 16 quarter-waves retire exactly one
// page per iteration, quarter-wave 4 * wid + quarter owning that row of it.
// Splits are page-aligned: of the np = ceil(pos / 16) pages that hold old
// rows, split s takes [s * ceil(np / DA_SPLIT), ...).  The page id of an
// iteration is workgroup-uniform and travels through scalar registers; the
// id of page i + 2 is fetched while the rows of page i + 1 are in flight, so
// the chain table -> address -> row load never waits inside the row prefetch.
//
// No table entry is trusted.  A sequence is ACTIVE only with
// 0 <= pos < 16 * pages_per_seq and every entry [b, 0 .. pos / 16] inside
// [0, num_pages); each workgroup establishes that with one strided pass and
// a workgroup vote before its first access to the pools or the RoPE table.
// An inactive sequence gets the neutral partial (phase 2 writes zeros) and
// nothing else.  Sequences may share pages for reading; two that append into
// one slot in the same step leave that slot undefined.

#include "mfma.h"  // uint4v
#include "paged_common.h"  // PG_ROWS, pg_valid, pg_id, PgKvSrc

template <int REP>
__global__ void __launch_bounds__(PG_THREADS)
paged_decode_attn_part(const short* __restrict__ qlin,
                       const short* __restrict__ klin,
                       const short* __restrict__ vlin,
                       short* __restrict__ kpages, short* __restrict__ vpages,
                       const int* __restrict__ block_table,
                       const float* __restrict__ cosp,
                       const float* __restrict__ sinp,
                       const long* __restrict__ pos_ptr,
                       float* __restrict__ part_o, float* __restrict__ part_ml,
                       int Hkv, int num_pages, int pages_per_seq, float scale,
                       int qstride, int kvstride) {
  DaCoord c;
  da_coord<REP, true>(c, pos_ptr, Hkv);
  const int tid = c.tid, hl = c.hl;
  const long pos = c.pos;
  // the position first: it bounds the pass over the table
  if (!da_active(pos, 1, PG_ROWS * pages_per_seq)) {  // the whole workgroup
    da_store_neutral(c.wg, REP, PG_THREADS, part_o, part_ml);
    return;
  }
  const int* tab = block_table + (long)c.b * pages_per_seq;
  const int last = (int)(pos / PG_ROWS);  // the page of the append
  int ok = 1;
  for (int j = tid; j <= last; j += PG_THREADS)
    ok &= pg_valid(tab[j], num_pages);
  if (!__syncthreads_and(ok)) {  // the same answer in every thread
    da_store_neutral(c.wg, REP, PG_THREADS, part_o, part_ml);
    return;
  }

  __shared__ float qr[REP][DA_D];
  __shared__ float knr[DA_D];
  __shared__ float vn[DA_D];
  __shared__ float merge_o[DA_SLOTS + 1][REP][DA_D];
  __shared__ float merge_ml[DA_SLOTS + 1][REP][2];

  // every split ropes the new k and loads v; only split 0 uses them
  if (tid < 64) {
    const float cs = cosp[pos * (DA_D / 2) + tid];
    const float sn = sinp[pos * (DA_D / 2) + tid];
    da_rope_q<REP>(qlin, qstride, c, cs, sn, qr);
    da_rope_pair(klin, (long)c.b * kvstride + c.kvh * DA_D, tid, cs, sn,
                 knr[tid], knr[tid + 64]);
  } else if (tid < 128) {
    int i = tid - 64;
    vn[i] = bits2f(vlin[(long)c.b * kvstride + c.kvh * DA_D + i]);
    vn[i + 64] = bits2f(vlin[(long)c.b * kvstride + c.kvh * DA_D + i + 64]);
  }
  __syncthreads();

  // elements of one page, and of this head's rows inside a page
  const long page_elems = (long)Hkv * PG_ROWS * DA_D;
  const long head_off = (long)c.kvh * PG_ROWS * DA_D;
  if (c.s == 0 && tid < DA_D) {
    const int pg = pg_id(tab, last, last + 1);
    const long row =
        pg * page_elems + head_off + (pos - (long)last * PG_ROWS) * DA_D;
    kpages[row + tid] = f2bits(knr[tid]);
    vpages[row + tid] = f2bits(vn[tid]);
  }

  const float s2 = scale * DA_LOG2E;
  float qv[REP][8], m_run[REP], l_run[REP], ov[REP][8];
  da_init_state<REP>(qr, hl, qv, m_run, l_run, ov);

  // pages [p0, p1) of the np that hold old rows; all of them <= last
  const int np = (int)((pos + PG_ROWS - 1) / PG_ROWS);
  const int per = (np + DA_SPLIT - 1) / DA_SPLIT;
  const int p0 = min(np, c.s * per);
  const int p1 = min(np, p0 + per);
  // this quarter-wave's row inside a page, this lane's dims inside the row
  const long lane_off = head_off + (4 * c.wid + c.quarter) * DA_D + 8 * hl;
  long r = (long)p0 * PG_ROWS + 4 * c.wid + c.quarter;  // masked at r >= pos

  const int pg_first = pg_id(tab, p0, p1);
  int pg_next = pg_id(tab, p0 + 1, p1);
  uint4v kp = {0, 0, 0, 0}, vp = {0, 0, 0, 0};
  if (p0 < p1 && r < pos) {
    const long a = pg_first * page_elems + lane_off;
    kp = *(const uint4v*)(kpages + a);
    vp = *(const uint4v*)(vpages + a);
  }
  for (int p = p0; p < p1; ++p) {
    // lands while the rows of page p + 1 load
    const int pg_next2 = pg_id(tab, p + 2, p1);
    const long rn = r + PG_ROWS;
    uint4v kpn = {0, 0, 0, 0}, vpn = {0, 0, 0, 0};
    if (p + 1 < p1 && rn < pos) {
      const long a = pg_next * page_elems + lane_off;
      kpn = *(const uint4v*)(kpages + a);
      vpn = *(const uint4v*)(vpages + a);
    }
    if (r < pos) {  // false only in the sequence's last page
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
        float pr = __builtin_amdgcn_exp2f(sc - m_new);
        m_run[g] = m_new;
        l_run[g] = l_run[g] * alpha + pr;
#pragma unroll
        for (int j = 0; j < 8; ++j) ov[g][j] = ov[g][j] * alpha + pr * vf[j];
      }
    }
    r = rn;
    kp = kpn;
    vp = vpn;
    pg_next = pg_next2;
  }

  da_store_partial<REP>(c, ov, m_run, l_run, merge_o, merge_ml);
  if (c.s == 0 && c.wid == 0)
    da_new_row_term<REP>(c, qv, knr, vn, s2, merge_o, merge_ml);
  __syncthreads();
  da_merge_store<REP>(c, merge_o, merge_ml, part_o, part_ml);
}

// Returns non-zero, launching nothing, outside da_launch_ok's contract (with
// Smax = 16 * pages_per_seq), with num_pages < 1 or pages_per_seq < 1, or
// with pools that break the 16-byte loads.
extern "C" int paged_decode_attn(const void* qlin, const void* klin,
                                 const void* vlin, void* kpages, void* vpages,
                                 const void* block_table, const void* cosp,
                                 const void* sinp, const void* pos_ptr,
                                 void* part_o, void* part_ml, void* outp,
                                 int B, int Hq, int Hkv, int num_pages,
                                 int pages_per_seq, float scale, int qstride,
                                 int kvstride, hipStream_t stream) {
  if (num_pages < 1 || pages_per_seq < 1 ||
      pages_per_seq > 0x7FFFFFFF / PG_ROWS)
    return 1;
  if (!da_launch_ok(B, Hq, Hkv, PG_ROWS * pages_per_seq, qstride, kvstride))
    return 1;
  if (((uintptr_t)kpages | (uintptr_t)vpages) % 16) return 1;
  da_for_rep(Hq / Hkv, [&](auto rep) {
    paged_decode_attn_part<decltype(rep)::value>
        <<<B * Hkv * DA_SPLIT, PG_THREADS, 0, stream>>>(
            (const short*)qlin, (const short*)klin, (const short*)vlin,
            (short*)kpages, (short*)vpages, (const int*)block_table,
            (const float*)cosp, (const float*)sinp, (const long*)pos_ptr,
            (float*)part_o, (float*)part_ml, Hkv, num_pages, pages_per_seq,
            scale, qstride, kvstride);
  });
  return decode_attn_merge_launch(part_o, part_ml, outp, B, 1, Hq, Hkv,
                                  stream);
}

// ---------------------------------------------------------------------------
// paged_kv_store: one thread per 16-byte piece (8 dims) of a K and of a V
// row.  Strides are in elements: (batch, head, seq); the last dim is dense.
// A row beyond the table, or whose entry names no pool page, is skipped.
// ---------------------------------------------------------------------------
#define PG_PIECES (DA_D / 8)  // 16-byte pieces per row

__global__ void __launch_bounds__(256)
paged_kv_store_kernel(PgKvSrc ksrc, PgKvSrc vsrc, short* __restrict__ kpages,
                      short* __restrict__ vpages,
                      const int* __restrict__ block_table, int B, int H,
                      int S, int num_pages, int pages_per_seq, long pos0) {
  const long per = (long)B * H * S * PG_PIECES;  // pieces of one operand
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * per) return;
  const bool is_v = idx >= per;
  if (is_v) idx -= per;
  const int piece = (int)(idx % PG_PIECES);
  long t = idx / PG_PIECES;
  const int sq = (int)(t % S);
  t /= S;
  const int h = (int)(t % H);
  const int b = (int)(t / H);

  const long row = pos0 + sq;
  const long j = row / PG_ROWS;
  if (j >= pages_per_seq) return;
  const int pg = block_table[(long)b * pages_per_seq + j];
  if (!pg_valid(pg, num_pages)) return;
  const PgKvSrc src = is_v ? vsrc : ksrc;
  short* pool = is_v ? vpages : kpages;
  const uint4v val =
      *(const uint4v*)(src.p + b * src.sb + h * src.sh + sq * src.ss +
                       8 * piece);
  *(uint4v*)(pool + (((long)pg * H + h) * PG_ROWS + (row - j * PG_ROWS)) *
                        DA_D + 8 * piece) = val;
}

// kstr / vstr: the four element strides (batch, head, seq, last) of k and v.
// Returns non-zero, launching nothing, on a contract violation: empty sizes,
// pos0 < 0, a non-dense last dim, or strides and pointers that break the
// 16-byte copies.
extern "C" int paged_kv_store(const void* k, const void* v, const long* kstr,
                              const long* vstr, void* kpages, void* vpages,
                              const void* block_table, int B, int H, int S,
                              int num_pages, int pages_per_seq, long pos0,
                              hipStream_t stream) {
  if (B < 1 || H < 1 || S < 1 || num_pages < 1 || pages_per_seq < 1 ||
      pos0 < 0)
    return 1;
  if (kstr[3] != 1 || vstr[3] != 1) return 1;
  for (int i = 0; i < 3; ++i)
    if (kstr[i] < 0 || vstr[i] < 0 || kstr[i] % 8 != 0 || vstr[i] % 8 != 0)
      return 1;
  if (((uintptr_t)k | (uintptr_t)v | (uintptr_t)kpages | (uintptr_t)vpages) %
      16)
    return 1;
  const long npiece = 2L * B * H * S * PG_PIECES;
  const long grid = (npiece + 255) / 256;
  if (grid > 0x7FFFFFFFL) return 1;
  const PgKvSrc ks = {(const short*)k, kstr[0], kstr[1], kstr[2]};
  const PgKvSrc vs = {(const short*)v, vstr[0], vstr[1], vstr[2]};
  paged_kv_store_kernel<<<(unsigned)grid, 256, 0, stream>>>(
      ks, vs, (short*)kpages, (short*)vpages, (const int*)block_table, B, H,
      S, num_pages, pages_per_seq, pos0);
  return 0;
}
