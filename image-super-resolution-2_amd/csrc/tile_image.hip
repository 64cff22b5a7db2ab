// The image-side kernels of the tiled C executor (ff_forward_image_u8, csrc/ff_executor.hip): what the plugin's _tiled_forward
// (models/team29_FreqFusion/io.py:87-164) does around `model(tile)` with host code and torch slices, as device work on uint8 images.
//   ff_tile_positions  the tile origins along one axis (io.py:87-91), pure host
//   ff_tile_cut_u8     uint8 HWC image -> one fp32 planar tile, u8 / 255 (the bits of ff_u8hwc_to_f32nchw + a slice copy)
//   ff_tile_ramps      the [4][st] edge-weight table of _ramp_table (io.py:97-113)
//   ff_tile_finish_u8  acc / max(wsum, 1e-8) -> clamp -> * 255 -> round half even -> uint8 HWC in ONE pass (the bits of
//                      ff_tile_normalize followed by ff_f32nchw_to_u8hwc); acc is only read
#include "ff_common.h"

extern "C" int ff_tile_positions(int n, int tile, int step, int* out, int cap) {
  if (n < tile || step < 1 || tile < 1 || !out) return -1;
  int cnt = 0, last = 0;
  for (long long p = 0; p < (long long)n - tile + 1; p += step) {        // range(0, max(n - tile + 1, 1), step); n >= tile here
    if (cnt >= cap) return -1;
    out[cnt++] = last = (int)p;
  }
  if (last + tile < n) {
    if (cnt >= cap) return -1;
    out[cnt++] = n - tile;
  }
  return cnt;
}

// img [H][W][3] uint8 -> out [3][th][tw], the tile at (y, x).  Byte loads: a row of the tile starts at byte 3 (y W + x), any alignment.
__global__ __launch_bounds__(256) void tile_cut_u8_kernel(const unsigned char* __restrict__ img, int W, int y, int x, int th, int tw,
                                                          float* __restrict__ out) {
  const long long plane = (long long)th * tw, total = 3 * plane;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i / plane);
    const long long r = i - c * plane;
    const int ty = (int)(r / tw), tx = (int)(r - (long long)ty * tw);
    out[i] = __fdiv_rn((float)img[((long long)(y + ty) * W + (x + tx)) * 3 + c], 255.0f);
  }
}

extern "C" int ff_tile_cut_u8(const unsigned char* img, int H, int W, int y, int x, int th, int tw, float* out, void* stream) {
  FF_CHECK_ARG(img && out, "ff_tile_cut_u8: null argument");
  FF_CHECK_ARG(H > 0 && W > 0 && th > 0 && tw > 0, "ff_tile_cut_u8: bad sizes (image %dx%d, tile %dx%d)", H, W, th, tw);
  FF_CHECK_ARG(y >= 0 && x >= 0 && (long long)y + th <= H && (long long)x + tw <= W,
               "ff_tile_cut_u8: the %dx%d tile at (%d,%d) leaves the %dx%d image", th, tw, y, x, H, W);
  long long nb = ((long long)3 * th * tw + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(tile_cut_u8_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, img, W, y, x, th, tw, out);
  FF_LAUNCH_CHECK("ff_tile_cut_u8");
  return FF_OK;
}

// tab [4][st]: row v = ones; bit 0: the first `blend` samples are ramp; bit 1: the last `blend` are 1 - ramp (written second, as
// _ramp_table does).  ramp = np.linspace(0, 1, blend, dtype=float32): (float)((double)i * step), the last element set to 1 when blend > 1.
__global__ __launch_bounds__(256) void tile_ramps_kernel(float* __restrict__ tab, int st, int blend, double step) {
  const long long total = (long long)4 * st;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int v = (int)(i / st), j = (int)(i - (long long)v * st);
    float w = 1.0f;
    int k = -1;
    bool falling = false;
    if ((v & 1) && j < blend) k = j;
    if ((v & 2) && j >= st - blend) { k = j - (st - blend); falling = true; }
    if (k >= 0) {
      const float ramp = (blend > 1 && k == blend - 1) ? 1.0f : (float)((double)k * step);
      w = falling ? __fsub_rn(1.0f, ramp) : ramp;
    }
    tab[i] = w;
  }
}

extern "C" int ff_tile_ramps(float* tab, int st, int blend, void* stream) {
  FF_CHECK_ARG(tab, "ff_tile_ramps: null argument");
  FF_CHECK_ARG(st > 0 && blend >= 0 && blend <= st, "ff_tile_ramps: blend %d must lie in [0, st = %d]", blend, st);
  const double step = blend > 1 ? 1.0 / (double)(blend - 1) : 0.0;
  long long nb = ((long long)4 * st + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(tile_ramps_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, tab, st, blend, step);
  FF_LAUNCH_CHECK("ff_tile_ramps");
  return FF_OK;
}

// ---- canvas -> uint8 image ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned finish_byte(float a, float w) {
  const float v = fminf(fmaxf(a / fmaxf(w, 1e-8f), 0.f), 1.f);          // tile_normalize_kernel, then f32nchw_to_u8hwc_kernel
  return (unsigned)(unsigned char)rintf(__fmul_rn(v, 255.0f));
}

// A plane starts P floats after the previous one, so only the first is known to be 16-byte aligned: the loads are dwordx4 on dword alignment.
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// VEC: a thread takes pixels 4g .. 4g+3 -- four 16-byte loads, twelve bytes packed into three dwords (out is 4-byte aligned, 12g keeps
// it so); the last P % 4 pixels go one per thread.  !VEC: one pixel per thread throughout (a destination that is not 4-byte aligned).
template <bool VEC>
__global__ __launch_bounds__(256) void tile_finish_u8_kernel(const float* __restrict__ acc, const float* __restrict__ wsum, long long P,
                                                             unsigned char* __restrict__ out) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nthr = (long long)gridDim.x * 256;
  const long long G = VEC ? P / 4 : 0;
  for (long long g = tid; g < G; g += nthr) {
    const long long p = 4 * g;
    const f32x4_a4 w = *reinterpret_cast<const f32x4_a4*>(wsum + p);
    const f32x4_a4 c0 = *reinterpret_cast<const f32x4_a4*>(acc + p);
    const f32x4_a4 c1 = *reinterpret_cast<const f32x4_a4*>(acc + P + p);
    const f32x4_a4 c2 = *reinterpret_cast<const f32x4_a4*>(acc + 2 * P + p);
    unsigned b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      b[3 * k] = finish_byte(c0[k], w[k]);
      b[3 * k + 1] = finish_byte(c1[k], w[k]);
      b[3 * k + 2] = finish_byte(c2[k], w[k]);
    }
    unsigned* o = reinterpret_cast<unsigned*>(out + 12 * g);
#pragma unroll
    for (int d = 0; d < 3; ++d) o[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
  }
  for (long long p = 4 * G + tid; p < P; p += nthr) {
    const float w = wsum[p];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * p + c] = (unsigned char)finish_byte(acc[c * P + p], w);
  }
}

extern "C" int ff_tile_finish_u8(const float* acc, const float* wsum, int H, int W, unsigned char* out, void* stream) {
  FF_CHECK_ARG(acc && wsum && out, "ff_tile_finish_u8: null argument");
  FF_CHECK_ARG(H > 0 && W > 0, "ff_tile_finish_u8: bad canvas size %dx%d", H, W);
  const long long P = (long long)H * W;
  const bool vec = ((uintptr_t)out & 3) == 0 && P >= 4;
  long long nb = ((vec ? P / 4 + 3 : P) + 255) / 256;
  if (nb > 8192) nb = 8192;
  if (vec) hipLaunchKernelGGL(tile_finish_u8_kernel<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, acc, wsum, P, out);
  else hipLaunchKernelGGL(tile_finish_u8_kernel<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, acc, wsum, P, out);
  FF_LAUNCH_CHECK("ff_tile_finish_u8");
  return FF_OK;
}
