// The image-side kernels of the tiled C executor (ff_forward_image_u8, csrc/ff_executor.hip): what the plugin's _tiled_forward
// (models/team29_FreqFusion/io.py:87-164) does around `model(tile)` with host code and torch slices, as device work on uint8 images.
//   ff_tile_positions  the tile origins along one axis (io.py:87-91), pure host
//   ff_tile_cut_u8     uint8 HWC image -> one fp32 planar tile, u8 / 255 (the bits of ff_u8hwc_to_f32nchw + a slice copy)
//   ff_tile_ramps      the [4][st] edge-weight table of _ramp_table (io.py:97-113)
//   ff_tile_finish_u8  acc / max(wsum, 1e-8) -> clamp -> * 255 -> round half even -> uint8 HWC in ONE pass (the bits of
//                      ff_tile_normalize followed by ff_f32nchw_to_u8hwc); acc is only read
// and the two kernels of the x8 self-ensemble on top of it (ff_forward_image_ens_u8):
//   ff_tile_cut_u8_d4  the same cut out of the TRANSFORMED image T_code(img), which is never materialised
//   ff_tile_fold_d4    one variant's canvas, normalised, mapped back and folded into the ensemble accumulator in ONE pass
#include "ff_common.h"
#include "d4_tile.inc"

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

// ---- the x8 self-ensemble's two kernels -----------------------------------------------------------------------------------------
// ff_d4_nchw's code (bit 0 flip(-1), then bit 1 flip(-2), then rot90(k = code >> 2)) as an index map, csrc/augment.hip:
//   even k: T[yo][xo] = img[revY ? H-1-yo : yo][revX ? W-1-xo : xo],  revY = v ^ (k == 2), revX = h ^ (k == 2)
//   odd k:  T[yo][xo] = img[ry ? H-1-xo : xo][rx ? W-1-yo : yo],      k = 1: ry = v, rx = !h;  k = 3: ry = !v, rx = h
// Either way the source PIXEL of T[yo][xo] is affine in (yo, xo): base + yo dy + xo dx, which the host works out once per launch.
// One thread takes one pixel: its three bytes are adjacent wherever the pixel lies, and each of its three stores goes to its own
// plane at the thread's index, so the fp32 side is coalesced for every code.  The byte side: |dx| = 1 walks a source row (forwards or
// backwards), |dx| = W (odd k) is a gather, one source row per lane -- the tile's source window is at most 3 t t bytes (48 KB at
// t = 128), which the caches hold, and it is read once.
__global__ __launch_bounds__(256) void tile_cut_u8_d4_kernel(const unsigned char* __restrict__ img, long long base, long long dy,
                                                             long long dx, int th, int tw, float* __restrict__ out) {
  const long long plane = (long long)th * tw;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < plane; r += (long long)gridDim.x * 256) {
    const int ty = (int)(r / tw), tx = (int)(r - (long long)ty * tw);
    const unsigned char* s = img + 3 * (base + ty * dy + tx * dx);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * plane + r] = __fdiv_rn((float)s[c], 255.0f);
  }
}

extern "C" int ff_tile_cut_u8_d4(const unsigned char* img, int H, int W, int code, int y, int x, int th, int tw, float* out,
                                 void* stream) {
  FF_CHECK_ARG(img && out, "ff_tile_cut_u8_d4: null argument");
  FF_CHECK_ARG(code >= 0 && code < 16, "ff_tile_cut_u8_d4: code %d outside 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)", code);
  FF_CHECK_ARG(H > 0 && W > 0 && th > 0 && tw > 0, "ff_tile_cut_u8_d4: bad sizes (image %dx%d, tile %dx%d)", H, W, th, tw);
  const int h = code & 1, v = (code >> 1) & 1, k = code >> 2, odd = k & 1;
  const int Ht = odd ? W : H, Wt = odd ? H : W;
  FF_CHECK_ARG(y >= 0 && x >= 0 && (long long)y + th <= Ht && (long long)x + tw <= Wt,
               "ff_tile_cut_u8_d4: the %dx%d tile at (%d,%d) leaves the %dx%d transformed image (code %d of a %dx%d image)", th, tw, y, x,
               Ht, Wt, code, H, W);
  long long base, dy, dx;
  if (!odd) {
    const int revY = v ^ (k >> 1), revX = h ^ (k >> 1);
    base = (revY ? (long long)(H - 1) * W : 0) + (revX ? W - 1 : 0);
    dy = revY ? -(long long)W : W;
    dx = revX ? -1 : 1;
  } else {
    const int ry = (k == 1) ? v : !v, rx = (k == 1) ? !h : h;
    base = (ry ? (long long)(H - 1) * W : 0) + (rx ? W - 1 : 0);
    dx = ry ? -(long long)W : W;
    dy = rx ? -1 : 1;
  }
  base += y * dy + x * dx;
  long long nb = ((long long)th * tw + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(tile_cut_u8_d4_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, img, base, dy, dx, th, tw, out);
  FF_LAUNCH_CHECK("ff_tile_cut_u8_d4");
  return FF_OK;
}

// The load hook of d4_tile for a canvas: an element of the source plane is acc / max(wsum, 1e-8), tile_normalize_kernel's arithmetic
// (csrc/elementwise.hip), one rounding.  wsum is ONE plane, indexed like the acc plane d4_tile was handed.
struct d4_load_norm {
  const float* __restrict__ wsum;
  __device__ __forceinline__ float at(const float* __restrict__ src, long long i) const { return src[i] / fmaxf(wsum[i], 1e-8f); }
  __device__ __forceinline__ f32x4 at4(const float* __restrict__ src, long long i) const {
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + i), w = *reinterpret_cast<const f32x4*>(wsum + i);
    return (f32x4){a[0] / fmaxf(w[0], 1e-8f), a[1] / fmaxf(w[1], 1e-8f), a[2] / fmaxf(w[2], 1e-8f), a[3] / fmaxf(w[3], 1e-8f)};
  }
};

// d4_rect_kernel (csrc/augment.hip) with the normalisation in the load: the blocks tile the OUTPUT planes of ens, three of them.
__global__ __launch_bounds__(256) void tile_fold_d4_kernel(const float* __restrict__ acc, const float* __restrict__ wsum,
                                                           float* __restrict__ ens, int Hc, int Wc, int code, int accum, float scale,
                                                           int tiles_x, int tiles_per_plane, int vec4) {
  __shared__ float tile[D4_TILE * D4_PITCH];
  const int plane = blockIdx.x / tiles_per_plane, t = blockIdx.x - plane * tiles_per_plane;
  const int ty0 = (t / tiles_x) * D4_TILE, tx0 = (t - (t / tiles_x) * tiles_x) * D4_TILE;      // origin of the OUTPUT tile
  const long long po = (long long)plane * Hc * Wc;
  d4_tile<true>(acc + po, ens + po, tile, Hc, Wc, code, ty0, tx0, vec4, accum, scale, d4_load_norm{wsum});
}

extern "C" int ff_tile_fold_d4(const float* acc, const float* wsum, int Hc, int Wc, int code, float* ens, int accum, float scale,
                               void* stream) {
  FF_CHECK_ARG(acc && wsum && ens, "ff_tile_fold_d4: null pointer");
  FF_CHECK_ARG(Hc > 0 && Wc > 0, "ff_tile_fold_d4: bad canvas size %dx%d", Hc, Wc);
  FF_CHECK_ARG(code >= 0 && code < 16, "ff_tile_fold_d4: code %d outside 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)", code);
  FF_CHECK_ARG(accum == 0 || accum == 1, "ff_tile_fold_d4: accum must be 0 or 1, got %d", accum);
  const long long P = (long long)Hc * Wc;
  const uintptr_t e0 = (uintptr_t)ens, e1 = e0 + 12 * (uintptr_t)P, a0 = (uintptr_t)acc, w0 = (uintptr_t)wsum;
  FF_CHECK_ARG(!(e0 < a0 + 12 * (uintptr_t)P && a0 < e1) && !(e0 < w0 + 4 * (uintptr_t)P && w0 < e1),
               "ff_tile_fold_d4: ens overlaps acc or wsum of the %dx%d canvas (the fold is not in place)", Hc, Wc);
  const int odd = (code >> 2) & 1;
  const int Hd = odd ? Wc : Hc, Wd = odd ? Hc : Wc;
  const int tiles_x = ff_cdiv(Wd, D4_TILE), tiles_y = ff_cdiv(Hd, D4_TILE);
  const long long blocks = 3LL * tiles_x * tiles_y;
  FF_CHECK_ARG(blocks < (1ll << 31), "ff_tile_fold_d4: %lld tiles of a %dx%d canvas exceed the grid limit", blocks, Hc, Wc);
  const int vec4 = (Wc % 4 == 0) && (((uintptr_t)acc | (uintptr_t)wsum | (uintptr_t)ens) & 15) == 0;
  hipLaunchKernelGGL(tile_fold_d4_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc, wsum, ens, Hc, Wc, code, accum,
                     scale, tiles_x, tiles_x * tiles_y, vec4);
  FF_LAUNCH_CHECK("ff_tile_fold_d4");
  return FF_OK;
}
