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

#include "d4_tile.inc"        // D4_TILE, d4_emit, d4_tile: shared with tile_fold_d4_kernel (csrc/tile_image.hip)

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
