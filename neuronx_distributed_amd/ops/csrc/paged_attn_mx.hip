// Paged MXFP8 KV cache for CDNA4: fused one-token decode attention that walks
// the quantized pages of each sequence through a block table, and the prefill
// store that quantizes into the pages.
//
//   paged_decode_attn_mx : RoPE(q,k) + quantize-and-append of the new K/V row
//                          into the sequence's page + flash-decode over its
//                          pages, GQA-grouped, split-KV; phase 2 is
//                          decode_attn_merge_launch (decode_attn.hip)
//   paged_mx_kv_store    : bf16 K, V (B, Hkv, S, D), any strides with a dense
//                          last dim -> payload + scales in the pages of rows
//                          [pos0, pos0 + S)
//
// Layouts (inference/kv_cache.py PagedMXKVCache): k_pages / v_pages uint8
// (num_pages, Hkv, PG_ROWS, 128), one e4m3fn byte per element; k_scale_pages
// / v_scale_pages uint8 (num_pages, Hkv, PG_ROWS, 4), biased e8m0, one per
// 32 dims: a row is pack_mx(quantize_mx(row)) as in decode_attn_mx.hip, 132
// bytes instead of 256.  block_table int32 (B, pages_per_seq) and pos_ptr as
// in paged_attn.hip, everything else as in decode_attn_common.h.
//
// The row mapping is decode_attn_mx.hip's: a quarter-wave owns a row, a lane
// 8 payload bytes inside ONE 32-block (one b64 load), and a quarter-wave
// takes DAMX_U = 2 rows per iteration from independent loads.  The 16
// quarter-waves then retire 32 rows = TWO pages per workgroup-iteration:
// unroll slot u reads row 4 * wid + quarter of page 2 i + u.  Both rows of a
// lane sit at the same offset inside their page, so the per-lane address is
// one 32-bit offset against two scalar page bases, for the payload and for
// the scale dword alike.  Splits are aligned to page pairs: of the
// ceil(np / 2) pairs that hold old rows, split s takes
// [s * ceil(pairs / DA_SPLIT), ...).  The two page ids of iteration i + 2 are
// fetched (scalar) while the rows of iteration i + 1 are in flight and
// iteration i computes, so table -> address -> row load never waits.
//
// Trust is paged_attn.hip's: a sequence is ACTIVE only with
// 0 <= pos < 16 * pages_per_seq and every entry [b, 0 .. pos / 16] inside
// [0, num_pages), established by one strided pass and a workgroup vote before
// the first access to a pool or the RoPE table; entries beyond pos / 16 are
// never read.  An inactive sequence gets the neutral partial and nothing
// else.
//
// Stale rows: a row at or beyond pos is never loaded, its registers hold
// zero bytes (value 0, scale 0).  Masking p alone would not do: a stale
// payload byte 0xFF / 0x7F is an e4m3 NaN and a stale scale byte 0xFF an
// infinite scale, and 0 * NaN would poison o.

#include "damx_append.h"
#include "mfma.h"
#include "paged_common.h"

#ifndef DAMX_U
#define DAMX_U 2       // rows per quarter-wave per iteration = pages of one
#endif
#define PGMX_SC (DA_D / 32)                  // scale bytes of a row

// the pool pages of iteration i (pages DAMX_U * i + u), 0 where the
// iteration lies outside [.., i1) or the page holds no old row (>= np)
struct PgmxIds {
  int p[DAMX_U];
};

__device__ __forceinline__ void pgmx_ids(const int* __restrict__ tab, int i,
                                         int i1, int np, PgmxIds& d) {
#pragma unroll
  for (int u = 0; u < DAMX_U; ++u)
    d.p[u] = pg_id(tab, DAMX_U * i + u, i < i1 ? np : 0);
}

template <int REP>
__global__ void __launch_bounds__(PG_THREADS)
paged_decode_attn_mx_part(const short* __restrict__ qlin,
                          const short* __restrict__ klin,
                          const short* __restrict__ vlin,
                          uint8_t* __restrict__ kpay,
                          uint8_t* __restrict__ ksc,
                          uint8_t* __restrict__ vpay,
                          uint8_t* __restrict__ vsc,
                          const int* __restrict__ block_table,
                          const float* __restrict__ cosp,
                          const float* __restrict__ sinp,
                          const long* __restrict__ pos_ptr,
                          float* __restrict__ part_o,
                          float* __restrict__ part_ml, int Hkv, int num_pages,
                          int pages_per_seq, float scale, int qstride,
                          int kvstride) {
  DaCoord c;
  da_coord<REP, true>(c, pos_ptr, Hkv);
  const int tid = c.tid, hl = c.hl;
  const int blk = hl >> 2;           // the 32-block the lane's dims lie in
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
  __shared__ short knb[DA_D];        // roped new K row, bf16 bits
  __shared__ short vnb[DA_D];        // new V row, bf16 bits
  __shared__ float knd[DA_D];        // the new rows as the pages hold them
  __shared__ float vnd[DA_D];
  __shared__ float merge_o[DA_SLOTS + 1][REP][DA_D];
  __shared__ float merge_ml[DA_SLOTS + 1][REP][2];

  // only split 0 ropes the new k and loads v
  if (tid < 64) {
    const float cs = cosp[pos * (DA_D / 2) + tid];
    const float sn = sinp[pos * (DA_D / 2) + tid];
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

  // bytes of one page in a payload pool and in a scale pool
  const long page_pay = (long)Hkv * PG_ROWS * DA_D;
  const long page_sc = (long)Hkv * PG_ROWS * PGMX_SC;
  if (c.s == 0) {
    const int pg = pg_id(tab, last, last + 1);
    const int row = c.kvh * PG_ROWS + (int)(pos - (long)last * PG_ROWS);
    if (tid < 8) {  // one thread per 32-block: 4 of K, 4 of V
      const long pay = pg * page_pay + (long)row * DA_D;
      const long sc = pg * page_sc + (long)row * PGMX_SC;
      if (tid < 4)
        damx_append_block(knb, tid, kpay + pay, ksc + sc, knd);
      else
        damx_append_block(vnb, tid - 4, vpay + pay, vsc + sc, vnd);
    }
  }

  const float s2 = scale * DA_LOG2E;
  float qv[REP][8], m_run[REP], l_run[REP], ov[REP][8];
  da_init_state<REP>(qr, hl, qv, m_run, l_run, ov);

  // page pairs [i0, i1) of those that hold old rows; every page < np <=
  // last + 1 was validated above
  const int np = (int)((pos + PG_ROWS - 1) / PG_ROWS);
  const int npair = (np + DAMX_U - 1) / DAMX_U;
  const int per = (npair + DA_SPLIT - 1) / DA_SPLIT;
  const int i0 = min(npair, c.s * per);
  const int i1 = min(npair, i0 + per);
  // this quarter-wave's row inside a page: the byte offsets of the lane's
  // dims and of the row's scale dword inside the page, one pair for every u
  const int slot = 4 * c.wid + c.quarter;
  const unsigned pay_off =
      (unsigned)((c.kvh * PG_ROWS + slot) * DA_D + 8 * hl);
  const unsigned sc_off = (unsigned)((c.kvh * PG_ROWS + slot) * PGMX_SC);

  // rows of iteration i: r + u * PG_ROWS, r = DAMX_U * PG_ROWS * i + slot;
  // a row at or beyond lim (pos, or 0 outside the split) is not loaded
  struct Rows {
    uint2v k[DAMX_U], v[DAMX_U];
    unsigned ks[DAMX_U], vs[DAMX_U];
  };
  auto load_rows = [&](const PgmxIds& ids, long r, long lim, Rows& t) {
#pragma unroll
    for (int u = 0; u < DAMX_U; ++u) {
      t.k[u] = uint2v{0, 0};
      t.v[u] = uint2v{0, 0};
      t.ks[u] = 0;
      t.vs[u] = 0;
      if (r + u * PG_ROWS < lim) {
        const long pb = ids.p[u] * page_pay, sb = ids.p[u] * page_sc;
        t.k[u] = *(const uint2v*)(kpay + pb + pay_off);
        t.v[u] = *(const uint2v*)(vpay + pb + pay_off);
        t.ks[u] = *(const unsigned*)(ksc + sb + sc_off);
        t.vs[u] = *(const unsigned*)(vsc + sb + sc_off);
      }
    }
  };

  long r = (long)i0 * (DAMX_U * PG_ROWS) + slot;
  PgmxIds id_cur, id_nxt;
  pgmx_ids(tab, i0, i1, np, id_cur);
  pgmx_ids(tab, i0 + 1, i1, np, id_nxt);
  Rows cur;
  load_rows(id_cur, r, i0 < i1 ? pos : 0, cur);
  for (int i = i0; i < i1; ++i) {
    // land while the rows of iteration i + 1 load
    PgmxIds id_nxt2;
    pgmx_ids(tab, i + 2, i1, np, id_nxt2);
    const long rn = r + DAMX_U * PG_ROWS;
    Rows nxt;
    load_rows(id_nxt, rn, i + 1 < i1 ? pos : 0, nxt);

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
      // rows at or beyond pos carry zero bytes; they are masked out here
      float sc[DAMX_U];
      float m_new = m_run[g];
#pragma unroll
      for (int u = 0; u < DAMX_U; ++u) {
        sc[u] = part[u * REP + g] * s2;
        if (r + u * PG_ROWS < pos) m_new = fmaxf(m_new, sc[u]);
      }
      const float alpha = __builtin_amdgcn_exp2f(m_run[g] - m_new);
      m_run[g] = m_new;
      l_run[g] *= alpha;
#pragma unroll
      for (int j = 0; j < 8; ++j) ov[g][j] *= alpha;
#pragma unroll
      for (int u = 0; u < DAMX_U; ++u) {
        const float p = (r + u * PG_ROWS < pos)
                            ? __builtin_amdgcn_exp2f(sc[u] - m_new) : 0.f;
        l_run[g] += p;
        const float pv = p * mxq_scale((cur.vs[u] >> (8 * blk)) & 0xff);
#pragma unroll
        for (int j = 0; j < 8; ++j) ov[g][j] += pv * vf[u][j];
      }
    }
    r = rn;
    cur = nxt;
    id_nxt = id_nxt2;
  }

  da_store_partial<REP>(c, ov, m_run, l_run, merge_o, merge_ml);
  __syncthreads();  // knd / vnd of the append are visible from here
  if (c.s == 0 && c.wid == 0)
    da_new_row_term<REP>(c, qv, knd, vnd, s2, merge_o, merge_ml);
  __syncthreads();
  da_merge_store<REP>(c, merge_o, merge_ml, part_o, part_ml);
}

// Returns non-zero, launching nothing, outside da_launch_ok's contract (with
// Smax = 16 * pages_per_seq), with num_pages < 1 or pages_per_seq < 1, with
// so many heads that a page's bytes pass 32 bits, or with pools that break
// the alignment of the loads and stores: 16 bytes for the payload pools (the
// append stores b128), 4 for the scale pools (a row's scales are one dword).
extern "C" int paged_decode_attn_mx(
    const void* qlin, const void* klin, const void* vlin, void* kpay,
    void* ksc, void* vpay, void* vsc, const void* block_table,
    const void* cosp, const void* sinp, const void* pos_ptr, void* part_o,
    void* part_ml, void* outp, int B, int Hq, int Hkv, int num_pages,
    int pages_per_seq, float scale, int qstride, int kvstride,
    hipStream_t stream) {
  if (num_pages < 1 || pages_per_seq < 1 ||
      pages_per_seq > 0x7FFFFFFF / PG_ROWS)
    return 1;
  if (!da_launch_ok(B, Hq, Hkv, PG_ROWS * pages_per_seq, qstride, kvstride))
    return 1;
  if (Hkv > 0x7FFFFFFF / (PG_ROWS * DA_D)) return 1;
  if (((uintptr_t)kpay | (uintptr_t)vpay) % 16) return 1;
  if (((uintptr_t)ksc | (uintptr_t)vsc) % 4) return 1;
  da_for_rep(Hq / Hkv, [&](auto rep) {
    paged_decode_attn_mx_part<decltype(rep)::value>
        <<<B * Hkv * DA_SPLIT, PG_THREADS, 0, stream>>>(
            (const short*)qlin, (const short*)klin, (const short*)vlin,
            (uint8_t*)kpay, (uint8_t*)ksc, (uint8_t*)vpay, (uint8_t*)vsc,
            (const int*)block_table, (const float*)cosp, (const float*)sinp,
            (const long*)pos_ptr, (float*)part_o, (float*)part_ml, Hkv,
            num_pages, pages_per_seq, scale, qstride, kvstride);
  });
  return decode_attn_merge_launch(part_o, part_ml, outp, B, 1, Hq, Hkv,
                                  stream);
}

// ---------------------------------------------------------------------------
// paged_mx_kv_store: one thread per 32-element block of K and of V, as
// mx_kv_store_kernel; the page lookup and the skip rule of
// paged_kv_store_kernel: a row beyond the table, or whose entry names no pool
// page, writes nothing.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
paged_mx_kv_store_kernel(PgKvSrc ksrc, PgKvSrc vsrc,
                         uint8_t* __restrict__ kpay,
                         uint8_t* __restrict__ ksc,
                         uint8_t* __restrict__ vpay,
                         uint8_t* __restrict__ vsc,
                         const int* __restrict__ block_table, int B, int H,
                         int S, int num_pages, int pages_per_seq, long pos0) {
  const long per = (long)B * H * S * PGMX_SC;  // blocks of one operand
  long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * per) return;
  const bool is_v = idx >= per;
  if (is_v) idx -= per;
  const int kb = (int)(idx % PGMX_SC);
  long t = idx / PGMX_SC;
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
  uint8_t* pay = is_v ? vpay : kpay;
  uint8_t* scl = is_v ? vsc : ksc;

  const s8v* in =
      (const s8v*)(src.p + b * src.sb + h * src.sh + sq * src.ss + 32 * kb);
  s8v v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = in[i];
  uint4v out[2];
  const int e = mxq_block32(v, out);
  const long prow = ((long)pg * H + h) * PG_ROWS + (row - j * PG_ROWS);
  uint4v* dst = (uint4v*)(pay + prow * DA_D + 32 * kb);
  dst[0] = out[0];
  dst[1] = out[1];
  scl[prow * PGMX_SC + kb] = (uint8_t)(e + 127);
}

// kstr / vstr: the four element strides (batch, head, seq, last) of k and v.
// Returns non-zero, launching nothing, on a contract violation: empty sizes,
// pos0 < 0, a non-dense last dim, or strides and pointers that break the
// 16-byte loads and stores.
extern "C" int paged_mx_kv_store(const void* k, const void* v,
                                 const long* kstr, const long* vstr,
                                 void* kpay, void* ksc, void* vpay, void* vsc,
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
  if (((uintptr_t)k | (uintptr_t)v | (uintptr_t)kpay | (uintptr_t)vpay) % 16)
    return 1;
  const long nblk = 2L * B * H * S * PGMX_SC;
  const long grid = (nblk + 255) / 256;
  if (grid > 0x7FFFFFFFL) return 1;
  const PgKvSrc ks = {(const short*)k, kstr[0], kstr[1], kstr[2]};
  const PgKvSrc vs = {(const short*)v, vstr[0], vstr[1], vstr[2]};
  paged_mx_kv_store_kernel<<<(unsigned)grid, 256, 0, stream>>>(
      ks, vs, (uint8_t*)kpay, (uint8_t*)ksc, (uint8_t*)vpay, (uint8_t*)vsc,
      (const int*)block_table, B, H, S, num_pages, pages_per_seq, pos0);
  return 0;
}
