// NAFBlock front half in one launch (nafnet_arch.py:88-98, the two bandwidth-bound HR levels C = 64 / 128):
//     t = conv1(LayerNorm2d(x))            1x1, C -> 2C          (was ff_token_linear: writes the 2C-wide tensor)
//     u = conv2(t)                         depth-wise 3x3, 2C    (was ff_dwconv3_gate_pool: reads it back 1.5x with halo)
//     g = u[:, :C] * u[:, C:]              SimpleGate
//     pool partials of g                   (SCA's global average pool)
// At 1024 x 1024 x 64 the two launches moved 805 + >805 MB for 268 MB in and 268 MB out.  Here a workgroup owns an 8 x 16 pixel tile:
// the 10 x 18 halo tokens are normalised and multiplied by W1 on the matrix cores (split-bf16, the same arithmetic as
// ff_token_linear: six 32-token m-tiles, one per wave, tokens stationary in registers), 32 gated channels at a time (their two
// 32-channel halves) go to LDS as fp32, the depth-wise taps read them there, and only g leaves the chip.  conv1 on the halo is
// recomputed (1.4x of a 17 GFLOP GEMM) -- the price for never materialising t.  The zero padding of conv2 applies to t, so tokens
// outside the image are stored as zeros, not as conv1(LayerNorm(0)).
// (included at the end of naf_fused.hip: it launches that file's pool_reduce_kernel, and device code is not relocatable here)

struct NafFrontParams {
  const float* x; int ldx;
  const float* gamma; const float* beta; float eps;
  const __bf16* w1;      // prep.pack_token_linear image: [NT = 2C/32][2 planes (hi, lo)][32 rows][KPAD = C]
  const float* b1;       // [2C]
  const float* wdw;      // [9][2C] tap-major
  const float* bdw;      // [2C]
  float* out; int ldo;   // [H*W][ldo], C channels
  float* part;           // [workgroups][C] sums of g over the workgroup's pixels
  int H, W, C, tiles_x, tiles_y;
};

#define NF_TY 8
#define NF_TX 16
#define NF_HW (NF_TX + 2)                 // halo tile width
#define NF_NTOK ((NF_TY + 2) * NF_HW)     // 180 halo tokens
// NF_MT = 6 m-tiles of 32 tokens (192 >= 180) and NF_TS = 68 floats per token row of the LDS tile: lds_layout.h, with the map
#define NF_BAD (-2147483647 - 1)          // row-offset sentinel: token outside the image / beyond the 180 halo tokens

#define NF_KERNEL naf_front_kernel
#define NF_IMAGES 0
#include "naf_front_kernel.inc"
#undef NF_KERNEL
#undef NF_IMAGES
#define NF_KERNEL naf_front_images_kernel
#define NF_IMAGES 1
#include "naf_front_kernel.inc"
#undef NF_KERNEL
#undef NF_IMAGES

extern "C" long long ff_naf_front_workspace(int H, int W, int C) {
  if (H <= 0 || W <= 0 || (C != 64 && C != 128)) return -1;
  return (long long)((H + NF_TY - 1) / NF_TY) * ((W + NF_TX - 1) / NF_TX) * C;
}

extern "C" long long ff_naf_front_images_workspace(int B, int H, int W, int C) {
  const long long one = ff_naf_front_workspace(H, W, C);
  if (B < 1 || one < 0) return -1;
  return (long long)B * one;
}

// The body of both entry points: B == 0 is ff_naf_front (one image, a grid of tiles), B >= 1 ff_naf_front_images (grid (tiles, B)).
static int naf_front_launch(const char* who, const float* x, int ldx, int B, int H, int W, int C, const float* ln_gamma, const float* ln_beta, float eps,
                            const void* w1_tiles, const float* b1, const float* dw_tapmajor, const float* dw_bias, float* out, int ldo,
                            float* pooled, float* work, long long work_floats, int nterms, void* stream) {
  FF_CHECK_ARG(nterms == 1 || nterms == 3, "%s: nterms must be 1 or 3", who);
  FF_CHECK_ARG(x && ln_gamma && ln_beta && w1_tiles && b1 && dw_tapmajor && dw_bias && out && pooled && work, "%s: null pointer", who);
  FF_CHECK_ARG(C == 64 || C == 128, "%s: built for 64 / 128 channels (got %d)", who, C);
  FF_CHECK_ARG(H > 0 && W > 0 && ldx >= C && ldx % 4 == 0 && ldo >= C && ldo % 4 == 0, "%s: bad dims", who);
  FF_CHECK_ARG((((uintptr_t)x) & 15) == 0 && (((uintptr_t)out) & 15) == 0 && (((uintptr_t)w1_tiles) & 15) == 0 && (((uintptr_t)b1) & 15) == 0 &&
               (((uintptr_t)dw_tapmajor) & 15) == 0 && (((uintptr_t)dw_bias) & 15) == 0 && (((uintptr_t)ln_gamma) & 15) == 0 && (((uintptr_t)ln_beta) & 15) == 0,
               "%s: 16-byte alignment required", who);
  FF_CHECK_ARG((long long)(NF_TY + 2) * W * ldx < (1LL << 31), "%s: row too long for the 32-bit offsets inside a tile", who);
  NafFrontParams p;
  p.x = x; p.ldx = ldx; p.gamma = ln_gamma; p.beta = ln_beta; p.eps = eps; p.w1 = (const __bf16*)w1_tiles; p.b1 = b1;
  p.wdw = dw_tapmajor; p.bdw = dw_bias; p.out = out; p.ldo = ldo; p.part = work; p.H = H; p.W = W; p.C = C;
  p.tiles_x = (W + NF_TX - 1) / NF_TX; p.tiles_y = (H + NF_TY - 1) / NF_TY;
  const long long nb = (long long)p.tiles_x * p.tiles_y;
  FF_CHECK_ARG(nb < (1LL << 31) && work_floats >= (B ? B : 1) * nb * C, "%s: workspace too small (%s_workspace)", who, who);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = nfr_lds(C);
  const float inv_hw = 1.0f / ((float)H * (float)W);
#define NF_LAUNCH(KERNEL, GRID, KSV, NTM)                                                                                    \
  do {                                                                                                                       \
    static ff_device_once once;                                                                                              \
    if (!ff_raise_lds(once, who, lds, FF_LDS_SAY_SIZE, &KERNEL<KSV, NTM>)) return FF_ERR_LAUNCH;                             \
    hipLaunchKernelGGL((KERNEL<KSV, NTM>), GRID, dim3(512), lds, st, p);                                                     \
  } while (0)
#define NF_LAUNCH_C(KERNEL, GRID)                                                                                            \
  do {                                                                                                                       \
    if (C == 64) { if (nterms == 3) NF_LAUNCH(KERNEL, GRID, 4, 3); else NF_LAUNCH(KERNEL, GRID, 4, 1); }                     \
    else { if (nterms == 3) NF_LAUNCH(KERNEL, GRID, 8, 3); else NF_LAUNCH(KERNEL, GRID, 8, 1); }                             \
  } while (0)
  if (!B) {
    NF_LAUNCH_C(naf_front_kernel, dim3((unsigned)nb));
    hipLaunchKernelGGL(pool_reduce_kernel, dim3((C + 15) / 16), dim3(256), 0, st, work, (int)nb, C, inv_hw, pooled);
  } else {
    NF_LAUNCH_C(naf_front_images_kernel, dim3((unsigned)nb, (unsigned)B));
    hipLaunchKernelGGL(pool_reduce_images_kernel, dim3((C + 15) / 16, (unsigned)B), dim3(256), 0, st, work, (int)nb, C, inv_hw, pooled);
  }
#undef NF_LAUNCH_C
#undef NF_LAUNCH
  FF_LAUNCH_CHECK(who);
  return FF_OK;
}

extern "C" int ff_naf_front(const float* x, int ldx, int H, int W, int C, const float* ln_gamma, const float* ln_beta, float eps,
                            const void* w1_tiles, const float* b1, const float* dw_tapmajor, const float* dw_bias, float* out, int ldo,
                            float* pooled, float* work, long long work_floats, int nterms, void* stream) {
  return naf_front_launch("ff_naf_front", x, ldx, 0, H, W, C, ln_gamma, ln_beta, eps, w1_tiles, b1, dw_tapmajor, dw_bias, out, ldo, pooled, work, work_floats, nterms, stream);
}

// B independent images x [B][H][W] (image stride H * W * ldx) in one launch: image b comes out with the bits of ff_naf_front on it alone.
// pooled [B][C]; work >= ff_naf_front_images_workspace(B, H, W, C) floats, laid out [B][tiles][C] in each image's single-image order.
extern "C" int ff_naf_front_images(const float* x, int ldx, int B, int H, int W, int C, const float* ln_gamma, const float* ln_beta, float eps,
                                   const void* w1_tiles, const float* b1, const float* dw_tapmajor, const float* dw_bias, float* out, int ldo,
                                   float* pooled, float* work, long long work_floats, int nterms, void* stream) {
  FF_CHECK_ARG(B >= 1 && B <= 65535, "ff_naf_front_images: B must be 1 .. 65535 (got %d)", B);
  return naf_front_launch("ff_naf_front_images", x, ldx, B, H, W, C, ln_gamma, ln_beta, eps, w1_tiles, b1, dw_tapmajor, dw_bias, out, ldo, pooled, work, work_floats, nterms, stream);
}

