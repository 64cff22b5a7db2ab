// One 64 x 64 tile of one plane under a symmetry of the square: the body shared by the D4 kernels of csrc/augment.hip (d4_nchw_kernel,
// d4_rect_kernel) and by tile_fold_d4_kernel of csrc/tile_image.hip.  Include after ff_common.h.
#pragma once

#define D4_TILE 64
#define D4_PITCH 65

// t = the permuted value:  accum 0: dst = t * scale;  accum 1: dst = (dst + t) * scale -- dst is read at the address, and with the
// width, of the store that follows it; the add is rounded before the multiply (no fma can form from add-then-multiply, and the
// contraction pragma keeps it so), hence scale == 1 leaves the sum's bits alone and a power-of-two scale is exact.
__device__ __forceinline__ float d4_emit(float t, float old, int accum, float scale) {
#pragma clang fp contract(off)
  const float s = accum ? old + t : t;
  return s * scale;
}

// The load hook of d4_tile: what a source element IS.  at(src, i) is element i of the plane src, at4 four of them from a 16-byte
// aligned i.  d4_load_plain reads the plane as it is (the D4 kernels: with it d4_tile compiles to what it was before the hook).
struct d4_load_plain {
  __device__ __forceinline__ float at(const float* __restrict__ src, long long i) const { return src[i]; }
  __device__ __forceinline__ f32x4 at4(const float* __restrict__ src, long long i) const { return *reinterpret_cast<const f32x4*>(src + i); }
};

// One 64 x 64 OUTPUT tile of one plane, src [Hs][Ws] -> dst [Hd][Wd] (even k: the same shape; odd k: [Ws][Hs]):
//   even k: dst[yo][xo] = src[revY ? Hs-1-yo : yo][revX ? Ws-1-xo : xo]
//   odd k:  dst[yo][xo] = src[ry ? Hs-1-xo : xo][rx ? Ws-1-yo : yo]
// The two axes of a ragged odd-k tile are clipped independently (ny against Hd, nx against Wd) and the input tile they select -- nx
// rows of ny columns -- is addressed with the input's own stride Ws, the output with Wd.
// EMIT = false stores the permuted value as it is: a pure copy, no multiply and no add, so denormals, negative zero and NaN
// payloads pass through untouched.  EMIT = true stores d4_emit(value, dst, accum, scale); dst is read only when accum is set, at
// the address, and with the width, of the store that follows it.
template <bool EMIT, class Load = d4_load_plain>
__device__ __forceinline__ void d4_tile(const float* __restrict__ src, float* __restrict__ dst, float* tile, int Hs, int Ws, int code,
                                        int ty0, int tx0, int vec4, int accum, float scale, const Load ld = Load()) {
  const int h = code & 1, v = (code >> 1) & 1, k = (code >> 2) & 3;
  const int tid = threadIdx.x;
  if ((k & 1) == 0) {
    const int H = Hs, W = Ws;
    const int revY = v ^ (k >> 1), revX = h ^ (k >> 1);
    if (vec4) {
      const int q = tid & 15, r0 = tid >> 4;                 // 16 float4 per 64-wide row, 16 rows per pass
      const int xo = tx0 + 4 * q;
      if (xo < W) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int yo = ty0 + r0 + 16 * p;
          if (yo < H) {
            const int yi = revY ? H - 1 - yo : yo;
            f32x4 a = ld.at4(src, (long long)yi * W + (revX ? W - 4 - xo : xo));
            if (revX) a = (f32x4){a[3], a[2], a[1], a[0]};
            f32x4* d = reinterpret_cast<f32x4*>(dst + (long long)yo * W + xo);
            if (EMIT) {
              f32x4 o = {0.f, 0.f, 0.f, 0.f};
              if (accum) o = *d;
#pragma unroll
              for (int e = 0; e < 4; ++e) a[e] = d4_emit(a[e], o[e], accum, scale);
            }
            *d = a;
          }
        }
      }
    } else {
      const int xo = tx0 + (tid & 63), r0 = tid >> 6;
      if (xo < W) {
        for (int p = 0; p < 16; ++p) {
          const int yo = ty0 + r0 + 4 * p;
          if (yo < H) {
            float* d = dst + (long long)yo * W + xo;
            const float a = ld.at(src, (long long)(revY ? H - 1 - yo : yo) * W + (revX ? W - 1 - xo : xo));
            *d = EMIT ? d4_emit(a, accum ? *d : 0.f, accum, scale) : a;
          }
        }
      }
    }
    return;
  }
  const int Hd = Ws, Wd = Hs;
  const int ry = (k == 1) ? v : !v, rx = (k == 1) ? !h : h;
  const int nx = min(D4_TILE, Wd - tx0), ny = min(D4_TILE, Hd - ty0);     // valid extent of the output tile, each axis on its own
  // input rows = images of the tile's output COLUMNS (nx of them, out of Hs), input columns = images of its ROWS (ny, out of Ws)
  const int iy0 = ry ? Hs - tx0 - nx : tx0, ix0 = rx ? Ws - ty0 - ny : ty0;
  const int lx = tid & 63, lr0 = tid >> 6;
#pragma unroll 4
  for (int p = 0; p < 16; ++p) {
    const int r = lr0 + 4 * p;                                            // input row iy0 + r (r < nx), input column ix0 + lx (lx < ny)
    if (r < nx && lx < ny) tile[r * D4_PITCH + lx] = ld.at(src, (long long)(iy0 + r) * Ws + ix0 + lx);
  }
  __syncthreads();
#pragma unroll 4
  for (int p = 0; p < 16; ++p) {
    const int r = lr0 + 4 * p;                                            // output row ty0 + r, output column tx0 + lx
    if (r < ny && lx < nx) {
      const int sy = ry ? nx - 1 - lx : lx;                               // input row of output column tx0 + lx, relative to iy0
      const int sx = rx ? ny - 1 - r : r;                                 // input column of output row ty0 + r, relative to ix0
      float* d = dst + (long long)(ty0 + r) * Wd + tx0 + lx;
      const float a = tile[sy * D4_PITCH + sx];
      *d = EMIT ? d4_emit(a, accum ? *d : 0.f, accum, scale) : a;
    }
  }
}
