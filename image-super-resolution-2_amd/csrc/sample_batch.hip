// One training micro-batch cut out of the resident image pool (isr2_amd.epoch.ImagePool / LiveEpoch): crop, u8 -> fp32 and the paired
// D4 augmentation of B samples, LR and HR, in ONE launch.  The reference does this per sample on the host (src/data/dataset.py:236-296
// reads and crops, augmentations.py:77-83 PairedRandomCrop, :128-135 / :169-171 flips and rot90) before collation.
//
//   pool  one byte buffer: every image uint8 HWC, packed back to back -- no base, no row pitch (3 w) and no `left` is aligned
//   desc  DEVICE int64 [B][8] = {lr_off, hr_off, h, w, top, left, code, 0}: byte offsets into the pool, LR image [h][w][3], its HR
//         partner [4h][4w][3], LR patch origin, code = bit 0 hflip | bit 1 vflip | bits 2-3 k of rot90 (ff_d4_nchw's meaning and order)
//   lr_out [B][3][p][p], hr_out [B][3][4p][4p] = u8 / 255 by IEEE division (the bits of ff_u8hwc_to_f32nchw and ff_crop_pairs_u8)
//
// With P the patch extent of a tensor (p or 4p) and (T, L) its origin (top, left or 4 top, 4 left), the index map of augment.hip on
// the square patch:
//   even k: out[yo][xo] = img[T + (revY ? P-1-yo : yo)][L + (revX ? P-1-xo : xo)]      revY = v ^ (k == 2), revX = h ^ (k == 2)
//   odd k:  out[yo][xo] = img[T + (ry ? P-1-xo : xo)][L + (rx ? P-1-yo : yo)]          k=1: ry = v, rx = !h;  k=3: ry = !v, rx = h
//
// One workgroup = one 64 x 64 OUTPUT tile of one sample of one of the two tensors, all three channels (a pixel's three bytes are
// adjacent and read once).  The code of a workgroup is uniform, so nothing diverges inside it.
//   even k: a thread converts four consecutive output pixels of a row -- twelve byte loads from one (mirrored) row segment -- and
//           stores one float4 into each plane; p % 4 != 0 or an unaligned output takes one pixel per thread and dword stores.
//   odd k:  the input tile is read by rows, parked in LDS as one packed dword per pixel (pitch 65: column reads hit 64 banks) and
//           read back by columns; the division happens after the LDS, and the output is written by rows of 64 floats per plane.
// Byte loads only, 64-bit offsets into the pool (DF2K's pool exceeds 2^31 bytes).  No atomics.  top / left are clamped here all the
// same as ops.sample_pairs_u8 checks them: no table can make the kernel leave the image it names.
#include "ff_common.h"

#define SB_TILE 64
#define SB_PITCH 65

__device__ __forceinline__ float sb_f(unsigned v) { return __fdiv_rn((float)v, 255.0f); }

template <bool VEC>
__global__ __launch_bounds__(256) void sample_pairs_u8_kernel(const unsigned char* __restrict__ pool, const long long* __restrict__ desc, int p,
                                                              float* __restrict__ lr_out, float* __restrict__ hr_out, int tiles_lr, int tx_lr,
                                                              int tiles_hr, int tx_hr) {
  __shared__ unsigned tile[SB_TILE * SB_PITCH];
  const int per = tiles_lr + tiles_hr;
  const int b = blockIdx.x / per, r_ = blockIdx.x - b * per;
  const bool is_hr = r_ >= tiles_lr;
  const int t = is_hr ? r_ - tiles_lr : r_, tiles_x = is_hr ? tx_hr : tx_lr;
  const int ty0 = (t / tiles_x) * SB_TILE, tx0 = (t - (t / tiles_x) * tiles_x) * SB_TILE;       // origin of the OUTPUT tile
  const long long* d = desc + (long long)b * 8;
  const int h = (int)d[2], w = (int)d[3];
  if (h < p || w < p) return;                                  // refused by the host; never index outside (uniform: no barrier is skipped)
  const int top = min(max((int)d[4], 0), h - p), left = min(max((int)d[5], 0), w - p);
  const int code = (int)d[6] & 15;
  const int s = is_hr ? 4 : 1;
  const int P = s * p;
  const long long pitch = 3ll * s * w;                         // bytes per image row
  const unsigned char* img = pool + (is_hr ? d[1] : d[0]) + (long long)(s * top) * pitch + 3ll * s * left;   // the patch's first byte
  const long long plane = (long long)P * P;
  float* out = (is_hr ? hr_out : lr_out) + (long long)b * 3 * plane;
  const int hf = code & 1, vf = (code >> 1) & 1, k = (code >> 2) & 3;
  const int tid = threadIdx.x;
  const int ny = min(SB_TILE, P - ty0), nx = min(SB_TILE, P - tx0);        // valid extent of the output tile
  if ((k & 1) == 0) {
    const int revY = vf ^ (k >> 1), revX = hf ^ (k >> 1);
    if (VEC) {                                                 // P % 4 == 0: nx is a multiple of 4, a group never straddles the edge
      const int q = tid & 15, r0 = tid >> 4;                   // 16 float4 per 64-wide row, 16 rows per pass
      const int xo = tx0 + 4 * q;
      if (4 * q < nx) {
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
          const int r = r0 + 16 * ps;
          if (r < ny) {
            const int yo = ty0 + r;
            const unsigned char* src = img + (long long)(revY ? P - 1 - yo : yo) * pitch + 3ll * (revX ? P - 4 - xo : xo);
            f32x4 v[3];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int c = 0; c < 3; ++c) v[c][revX ? 3 - j : j] = sb_f(src[3 * j + c]);
            float* dst = out + (long long)yo * P + xo;
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(dst + c * plane) = v[c];
          }
        }
      }
    } else {
      const int lx = tid & 63, r0 = tid >> 6;
      if (lx < nx) {
        const int xo = tx0 + lx;
        const long long sx = 3ll * (revX ? P - 1 - xo : xo);
        for (int ps = 0; ps < 16; ++ps) {
          const int r = r0 + 4 * ps;
          if (r < ny) {
            const int yo = ty0 + r;
            const unsigned char* src = img + (long long)(revY ? P - 1 - yo : yo) * pitch + sx;
            float* dst = out + (long long)yo * P + xo;
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c * plane] = sb_f(src[c]);
          }
        }
      }
    }
    return;
  }
  const int ry = (k == 1) ? vf : !vf, rx = (k == 1) ? !hf : hf;
  // input rows = images of the tile's output COLUMNS (nx of them), input columns = images of its ROWS (ny of them)
  const int iy0 = ry ? P - tx0 - nx : tx0, ix0 = rx ? P - ty0 - ny : ty0;
  const int lx = tid & 63, lr0 = tid >> 6;
#pragma unroll 4
  for (int ps = 0; ps < 16; ++ps) {
    const int r = lr0 + 4 * ps;                                // input row iy0 + r (r < nx), input column ix0 + lx (lx < ny)
    if (r < nx && lx < ny) {
      const unsigned char* src = img + (long long)(iy0 + r) * pitch + 3ll * (ix0 + lx);
      tile[r * SB_PITCH + lx] = (unsigned)src[0] | ((unsigned)src[1] << 8) | ((unsigned)src[2] << 16);
    }
  }
  __syncthreads();
#pragma unroll 4
  for (int ps = 0; ps < 16; ++ps) {
    const int r = lr0 + 4 * ps;                                // output row ty0 + r, output column tx0 + lx
    if (r < ny && lx < nx) {
      const int sy = ry ? nx - 1 - lx : lx;                    // input row of output column tx0 + lx, relative to iy0
      const int sx = rx ? ny - 1 - r : r;                      // input column of output row ty0 + r, relative to ix0
      const unsigned px = tile[sy * SB_PITCH + sx];
      float* dst = out + (long long)(ty0 + r) * P + tx0 + lx;
      dst[0] = sb_f(px & 255u);
      dst[plane] = sb_f((px >> 8) & 255u);
      dst[2 * plane] = sb_f(px >> 16);
    }
  }
}

extern "C" int ff_sample_pairs_u8(const unsigned char* pool, const long long* desc, int B, int p, float* lr_out, float* hr_out,
                                  void* stream) {
  FF_CHECK_ARG(pool && desc && lr_out && hr_out && B >= 1 && p >= 1,
               "ff_sample_pairs_u8: null pointer or bad sizes (B %d, p %d: both must be >= 1)", B, p);
  FF_CHECK_ARG(p <= 8192 && B <= (1 << 20), "ff_sample_pairs_u8: sizes out of range (B %d, p %d)", B, p);
  const int tx_lr = ff_cdiv(p, SB_TILE), tx_hr = ff_cdiv(4 * p, SB_TILE);
  const long long blocks = (long long)B * ((long long)tx_lr * tx_lr + (long long)tx_hr * tx_hr);
  FF_CHECK_ARG(blocks < (1ll << 31), "ff_sample_pairs_u8: %lld tiles exceed the grid limit", blocks);
  // float4 stores need rows of whole groups in BOTH tensors (p % 4 == 0) and 16-byte aligned outputs; else the dword form
  const bool vec = p % 4 == 0 && ((((uintptr_t)lr_out) | ((uintptr_t)hr_out)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(sample_pairs_u8_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pool, desc, p, lr_out, hr_out,
                       tx_lr * tx_lr, tx_lr, tx_hr * tx_hr, tx_hr);
  else
    hipLaunchKernelGGL(sample_pairs_u8_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pool, desc, p, lr_out, hr_out,
                       tx_lr * tx_lr, tx_lr, tx_hr * tx_hr, tx_hr);
  FF_LAUNCH_CHECK("ff_sample_pairs_u8");
  return FF_OK;
}
