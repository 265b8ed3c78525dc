// What the multi-token decode-attention kernels share: chunk_attn.hip (dense
// bf16 and MXFP8 caches) and paged_chunk_attn.hip (bf16 and MXFP8 page
// pools).  The per-wave staging of a 32-row tile as the dual-use LDS image of
// mfma.h, with the dequantizing form for MXFP8 rows, the RoPE of a query
// fragment and the launch contract.  Each file keeps its own walk over the
// cache (ca_load there, pc_load here) and its own kernels.
#pragma once

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

// compiler-level ordering of one wave's LDS writes and reads (the hardware
// keeps a wave's LDS operations in order)
__device__ __forceinline__ void ca_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The registers of one wave's share of a 32-row tile between its global loads
// and its LDS writes.  bf16: lane l, step i owns row 4i + (l >> 4), 16-byte
// chunk l & 15.  MXFP8: step i owns row 8i + (l >> 3), payload bytes
// 16 (l & 7) ..+15, and the row's four scale bytes as one dword.
template <bool MX> struct CaRegs;
template <> struct CaRegs<false> { uint4v k[8], v[8]; };
template <> struct CaRegs<true> { uint4v k[4], v[4]; unsigned ks[4], vs[4]; };

__device__ __forceinline__ uint4v ca_sel(bool ok, uint4v x) {
  const uint4v z = {0, 0, 0, 0};
  return ok ? x : z;
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

// The launch contract: da_launch_ok's, T in [2, 8] with Smax >= T, strides
// that hold a row and keep the 16-byte loads aligned.
static inline bool ca_launch_ok(const void* q, const void* k, const void* v,
                                const void* cosp, const void* sinp, int B,
                                int T, int Hq, int Hkv, int Smax, long q_bs,
                                long q_ts, long kv_bs, long kv_ts) {
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
