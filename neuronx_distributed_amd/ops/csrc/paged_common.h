// What the one-token kernels over a paged KV cache share: paged_attn.hip
// (bf16 pages) and paged_attn_mx.hip (MXFP8 pages).  The page geometry, the
// test of a table entry, the scalar fetch of a page id and the strided
// source of the prefill stores.
#pragma once

#include "decode_attn_common.h"

#define PG_ROWS DA_SLOTS
#define PG_THREADS (DA_WAVES * 64)

// a table entry that names a pool page
__device__ __forceinline__ bool pg_valid(int e, int num_pages) {
  return (unsigned)e < (unsigned)num_pages;
}

// The pool page of page p of a sequence (tab its table row), 0 at p >= p1.
// Workgroup-uniform: one scalar load, the id stays in a scalar register.
__device__ __forceinline__ int pg_id(const int* __restrict__ tab, int p,
                                     int p1) {
  return p < p1 ? __builtin_amdgcn_readfirstlane(tab[p]) : 0;
}

// bf16 K or V (B, Hkv, S, D) of a prefill store; strides in elements:
// (batch, head, seq), the last dim is dense
struct PgKvSrc {
  const short* p;
  long sb, sh, ss;
};
