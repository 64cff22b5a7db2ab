// Paired training augmentation on the device: the eight symmetries of the square (D4) applied per SAMPLE to a planar batch.
// The reference augments each sample on the host before collation (src/data/cached_dataset.py:240-268):
//   hflip = flip(dims=[-1]) (p 0.5), then vflip = flip(dims=[-2]) (p 0.5), then rot90(k, dims=[-2,-1]) with k in 0..3,
// the same transform for lr, hr, the three expert images and the three feature maps.  Here the loader uploads the batch as read and
// ONE launch per tensor permutes it: codes[b] = bit 0 hflip | bit 1 vflip | bits 2-3 k.
//
// Composition, as an index map (out is [Ho][Wo], Ho = H and Wo = W; odd k needs H == W so that a batch keeps one shape):
//   rot90 k=1: r[i][j] = t[j][W-1-i]    k=2: r[i][j] = t[H-1-i][W-1-j]    k=3: r[i][j] = t[H-1-j][i]
//   t = vflip(hflip(in)): t[y][x] = in[v ? H-1-y : y][h ? W-1-x : x]
// so even k is a copy with rows and / or columns reversed (revY = v ^ (k==2), revX = h ^ (k==2)) and odd k is a transpose with
// reversals: out[yo][xo] = in[ry ? N-1-xo : xo][rx ? N-1-yo : yo], k=1: ry = v, rx = !h;  k=3: ry = !v, rx = h.
//
// A pure permutation, HBM-bound.  One block moves one 64 x 64 tile of one plane:
//   even k: each thread moves float4s of a row (a reversed row reads the mirrored float4 and swaps its lanes), so both sides are
//           16-byte accesses of whole 256-byte row segments; W % 4 != 0 or unaligned bases take the dword form of the same loop.
//   odd k:  the input tile is read by rows (a wave = one 256-byte row segment), parked in LDS with a pitch of 65 dwords and read back
//           by columns: lane l of a wave reads dword 65 l + c, bank (l + c) mod 64 -- all 64 banks, no conflict -- and the output is
//           written by rows again.
// The code of a block is uniform (one sample per plane), so there is no divergence inside a block.
#include "ff_common.h"

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

// One 64 x 64 OUTPUT tile of one plane, src [Hs][Ws] -> dst [Hd][Wd] (even k: the same shape; odd k: [Ws][Hs]):
//   even k: dst[yo][xo] = src[revY ? Hs-1-yo : yo][revX ? Ws-1-xo : xo]
//   odd k:  dst[yo][xo] = src[ry ? Hs-1-xo : xo][rx ? Ws-1-yo : yo]
// The two axes of a ragged odd-k tile are clipped independently (ny against Hd, nx against Wd) and the input tile they select -- nx
// rows of ny columns -- is addressed with the input's own stride Ws, the output with Wd.
// EMIT = false stores the permuted value as it is: a pure copy, no multiply and no add, so denormals, negative zero and NaN
// payloads pass through untouched.  EMIT = true stores d4_emit(value, dst, accum, scale); dst is read only when accum is set, at
// the address, and with the width, of the store that follows it.
template <bool EMIT>
__device__ __forceinline__ void d4_tile(const float* __restrict__ src, float* __restrict__ dst, float* tile, int Hs, int Ws, int code,
                                        int ty0, int tx0, int vec4, int accum, float scale) {
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
            f32x4 a = *reinterpret_cast<const f32x4*>(src + (long long)yi * W + (revX ? W - 4 - xo : xo));
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
            const float a = src[(long long)(revY ? H - 1 - yo : yo) * W + (revX ? W - 1 - xo : xo)];
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
    if (r < nx && lx < ny) tile[r * D4_PITCH + lx] = src[(long long)(iy0 + r) * Ws + ix0 + lx];
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

// per-SAMPLE codes on square-or-even-k planes: the training augmentation, a pure copy (EMIT off)
__global__ __launch_bounds__(256) void d4_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int H, int W,
                                                      const int* __restrict__ codes, int tiles_x, int tiles_per_plane, int vec4) {
  __shared__ float tile[D4_TILE * D4_PITCH];
  const int plane = blockIdx.x / tiles_per_plane, t = blockIdx.x - plane * tiles_per_plane;
  const int ty0 = (t / tiles_x) * D4_TILE, tx0 = (t - (t / tiles_x) * tiles_x) * D4_TILE;      // origin of the OUTPUT tile
  int code = codes[plane / C] & 15;
  if (H != W) code &= ~4;                                    // odd k on a non-square plane is refused by the host; never index outside
  d4_tile<false>(in + (long long)plane * H * W, out + (long long)plane * H * W, tile, H, W, code, ty0, tx0, vec4, 0, 1.f);
}

extern "C" int ff_d4_nchw(const float* in, float* out, int B, int C, int H, int W, const int* codes, void* stream) {
  FF_CHECK_ARG(in && out && codes, "ff_d4_nchw: null pointer");
  FF_CHECK_ARG(in != out, "ff_d4_nchw: the permutation is not in place (in == out)");
  FF_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "ff_d4_nchw: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
  const int tiles_x = ff_cdiv(W, D4_TILE), tiles_y = ff_cdiv(H, D4_TILE);
  const long long blocks = (long long)B * C * tiles_x * tiles_y;
  FF_CHECK_ARG(blocks < (1ll << 31), "ff_d4_nchw: %lld tiles exceed the grid limit", blocks);
  const int vec4 = (W % 4 == 0) && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
  hipLaunchKernelGGL(d4_nchw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, out, C, H, W, codes, tiles_x,
                     tiles_x * tiles_y, vec4);
  FF_LAUNCH_CHECK("ff_d4_nchw");
  return FF_OK;
}

// ---- one symmetry on RECTANGULAR planes, with fused accumulation (geometric self-ensemble, model.FreqFusionHIP.self_ensemble) ----
// ONE code for the whole launch, any Hs x Ws: even k keeps the plane's shape, odd k writes [Ws][Hs].  The blocks tile the OUTPUT plane;
// d4_tile with EMIT on.
__global__ __launch_bounds__(256) void d4_rect_kernel(const float* __restrict__ in, float* __restrict__ out, int Hs, int Ws, int code,
                                                      int accum, float scale, int tiles_x, int tiles_per_plane, int vec4) {
  __shared__ float tile[D4_TILE * D4_PITCH];
  const int plane = blockIdx.x / tiles_per_plane, t = blockIdx.x - plane * tiles_per_plane;
  const int ty0 = (t / tiles_x) * D4_TILE, tx0 = (t - (t / tiles_x) * tiles_x) * D4_TILE;      // origin of the OUTPUT tile
  d4_tile<true>(in + (long long)plane * Hs * Ws, out + (long long)plane * Hs * Ws, tile, Hs, Ws, code, ty0, tx0, vec4, accum, scale);
}

extern "C" int ff_d4_rect_nchw(const float* src, float* dst, int B, int C, int Hs, int Ws, int code, int accum, float scale,
                               void* stream) {
  FF_CHECK_ARG(src && dst, "ff_d4_rect_nchw: null pointer");
  FF_CHECK_ARG(src != dst, "ff_d4_rect_nchw: the permutation is not in place (src == dst)");
  FF_CHECK_ARG(B > 0 && C > 0 && Hs > 0 && Ws > 0, "ff_d4_rect_nchw: bad shape B=%d C=%d Hs=%d Ws=%d", B, C, Hs, Ws);
  FF_CHECK_ARG(code >= 0 && code < 16, "ff_d4_rect_nchw: code %d outside 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)", code);
  FF_CHECK_ARG(accum == 0 || accum == 1, "ff_d4_rect_nchw: accum must be 0 or 1, got %d", accum);
  const int odd = (code >> 2) & 1;
  const int Hd = odd ? Ws : Hs, Wd = odd ? Hs : Ws;
  const int tiles_x = ff_cdiv(Wd, D4_TILE), tiles_y = ff_cdiv(Hd, D4_TILE);
  const long long blocks = (long long)B * C * tiles_x * tiles_y;
  FF_CHECK_ARG(blocks < (1ll << 31), "ff_d4_rect_nchw: %lld tiles exceed the grid limit", blocks);
  const int vec4 = (Ws % 4 == 0) && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  hipLaunchKernelGGL(d4_rect_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src, dst, Hs, Ws, code, accum, scale,
                     tiles_x, tiles_x * tiles_y, vec4);
  FF_LAUNCH_CHECK("ff_d4_rect_nchw");
  return FF_OK;
}
