// Layout probe for the dual-use LDS image of mfma.h (img_off / img_row_read
// / img_tr_read).  Launch with ONE wave (64 threads).
//
// Stages one 32x128 tile of 16-bit values in the image exactly as the
// flash-attention backward kernels do (16-byte chunks through img_off) and
// dumps, for the 32x32x16 operand,
//   row_out[c][lane][j]      c = 0..7           : A-operand row reads
//   tr_out[ck][nb][lane][j]  ck = 0..1, nb = 0..3: B-operand transposed reads
// The caller fills the tile with distinct bit patterns, so every lane /
// element can be checked against the index map computed on the host.

#include "common.h"
#include "mfma.h"

extern "C" __global__ void __launch_bounds__(64)
probe_lds_image_kernel(const short* __restrict__ tile,
                       short* __restrict__ row_out,
                       short* __restrict__ tr_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int col = lane & 31;
  const int hi = lane >> 5;
  // 32 rows x 16 chunks = 512 chunks, 8 per lane
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int p = lane + i * 64;
    int row = p >> 4, ch = p & 15;
    *(uint4v*)(smem + img_off(row, ch)) =
        *(const uint4v*)(tile + row * 128 + ch * 8);
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 8; ++c)
    *(uint4v*)(row_out + (c * 64 + lane) * 8) =
        img_row_read(smem, img_row_base(col, hi), c);
#pragma unroll
  for (int ck = 0; ck < 2; ++ck)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
      *(uint4v*)(tr_out + ((ck * 4 + nb) * 64 + lane) * 8) =
          img_tr_read(smem, img_tr_base(lane), ck * 16, nb * 32);
}

extern "C" void run_probe_lds_image(const void* tile, void* row_out,
                                    void* tr_out, hipStream_t s) {
  probe_lds_image_kernel<<<1, 64, 32 * IMG_ROW_B, s>>>(
      (const short*)tile, (short*)row_out, (short*)tr_out);
}
