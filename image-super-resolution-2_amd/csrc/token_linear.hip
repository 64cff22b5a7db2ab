// Token-stationary linear layer for the K <= 192 transformer projections:
//     out[token][n] = res[token][n] + res2[token][n]*rs2[n] + act( LayerNorm?(x)[token] . W[n] + bias[n] )
// (hat_arch.py:172 qkv after norm1 :272, :194 proj; dat_arch.py:501,559 qkv/proj, :163 fc1 after norm2 :735).
// These layers move 140-190 MB for 4-13 GFLOP at 65 536 tokens: they are HBM-bound, and the generic tiled GEMM
// (conv_gemm_bf16.hip) runs them latency-bound at 1.5 TB/s because K = 180 is only six 32-deep chunks per tile.
// Here a wave keeps its 32 tokens' (optionally layer-normalised) rows in REGISTERS as split-bf16 MFMA B operands
// for the whole kernel (x is read from HBM exactly once, LayerNorm costs no extra pass), the weight matrix streams
// through a two-slot LDS ring by LDS-DMA in 32-row tiles shared by the 8 waves, and every 32(n) x 32(token)
// accumulator tile is transposed through a wave-private LDS patch so stores are 128-byte row segments.
// Dataflow per n-tile: OUT^T[n][token] = W_tile . X^T   (A = W rows from LDS, B = X fragments), 36 MFMAs (bf16x3).
#include "ff_common.h"

// KS = k-steps of 16 (K padded to 16*KS): 12 for the 180-wide transformers, 4 / 8 for NAFNet's 64 / 128 channels.
// Per W row: 2*KS data slots of 16 bytes + 1 pad slot; a tile (32 rows, hi + lo planes) is 2*32*(2KS+1)/64 DMA pieces
// (25 / 17 / 9 -- always integral).

struct TokenLinParams {
  const float* x; float* out;
  const float* gamma; const float* beta;   // NULL: no LayerNorm
  const __bf16* w;                         // [NT][2 planes][32][192], rows >= N zero
  const float* bias;                       // [NT*32] zero padded (or NULL)
  const float* res; const float* res2; const float* rs2;
  float* xn; int ldxn;                     // optional side output: the LayerNorm'ed rows (NULL: not written)
  float* stats; int st_lo, st_hi; float st_eps;   // optional side output: per token (mean, rstd) of OUTPUT channels [st_lo, st_hi)
  // GATED prologue (DAT adaptive interaction, dat_arch.py:541-556 / :649-664): the GEMM input is  x * cm[channel] + x2 * sm[token],
  // sm = sigmoid(gw2 . gelu(GW1 x + gb1) + gb2) computed from x itself (GW1: 180 -> 11, BatchNorm folded)
  const float* x2; int ldx2; const float* cm; const float* gw1t; const float* gb1; const float* gw2; float gb2;
  long long M;
  int ldx, ldo, ldr, ldr2, K, N, NT, act;
  float eps;
  int wpi;                                 // token_linear_images_kernel: 256-token workgroups per image (grid (wpi, images), cm [images][K])
};

// NTERMS = 3: split-bf16 products hi*lo + lo*hi + hi*hi (fp32-grade); NTERMS = 1: plain bf16 (hi*hi only: a third of the MFMAs, no lo
// fragments built or read; the weight image keeps its lo plane, unused).
#ifndef TL_GELU_SIG
#define TL_GELU_SIG 1
#endif
#define TL_KERNEL token_linear_kernel
#define TL_IMAGES 0
#define TL_OUT16 0
#include "token_linear_kernel.inc"
#undef TL_KERNEL
#undef TL_IMAGES
#define TL_KERNEL token_linear_images_kernel       // GATED rows of B images, cm [B][K] (ff_token_linear_gated_images)
#define TL_IMAGES 1
#include "token_linear_kernel.inc"
#undef TL_KERNEL
#undef TL_IMAGES
#undef TL_OUT16
#define TL_KERNEL token_linear_rows16_kernel       // column-scaled bf16 rows out (ff_token_linear_rows16)
#define TL_IMAGES 0
#define TL_OUT16 1
#include "token_linear_kernel.inc"
#undef TL_KERNEL
#undef TL_IMAGES
#undef TL_OUT16


extern "C" int ff_token_linear(const float* x, int ldx, float* out, int ldo, long long M, int K, int kpad, int N, int n_tiles,
                               const float* gamma, const float* beta, float eps, const void* w_tiles,
                               const float* bias_padded, int act, const float* res, int ldr, const float* res2, int ldr2,
                               const float* res2_scale, float* xn_out, int ldxn, float* stats_out, int stat_lo, int stat_hi,
                               float stat_eps, int nterms, void* stream) {
  FF_CHECK_ARG(nterms == 1 || nterms == 3, "ff_token_linear: nterms must be 1 (plain bf16) or 3 (split bf16)");
  FF_CHECK_ARG(x && out && w_tiles, "ff_token_linear: null pointer");
  FF_CHECK_ARG(M > 0 && K > 0 && K <= 192 && K % 4 == 0 && N > 0 && n_tiles * 32 >= N, "ff_token_linear: needs K <= 192 (K %% 4 == 0), n_tiles*32 >= N");
  FF_CHECK_ARG(kpad == 64 || kpad == 128 || kpad == 192, "ff_token_linear: kpad must be 64, 128 or 192");
  FF_CHECK_ARG(kpad >= K, "ff_token_linear: kpad < K");
  FF_CHECK_ARG(ldx >= K && ldx % 4 == 0 && ldo >= N && (((uintptr_t)x) & 15) == 0, "ff_token_linear: x rows must be 16-byte aligned");
  FF_CHECK_ARG((gamma == nullptr) == (beta == nullptr), "ff_token_linear: gamma/beta come together");
  FF_CHECK_ARG((((uintptr_t)w_tiles) & 15) == 0 && (!gamma || ((((uintptr_t)gamma) & 15) == 0 && (((uintptr_t)beta) & 15) == 0)), "ff_token_linear: weights / gamma / beta must be 16-byte aligned");
  FF_CHECK_ARG(!res || ldr >= N, "ff_token_linear: ldr too small");
  FF_CHECK_ARG(!res2 || (ldr2 >= N && res2_scale), "ff_token_linear: res2 needs ldr2 >= N and a scale vector");
  FF_CHECK_ARG(!xn_out || (gamma && ldxn >= K && ldxn % 4 == 0 && (((uintptr_t)xn_out) & 15) == 0), "ff_token_linear: xn_out needs LayerNorm parameters and 16-byte aligned rows");
  TokenLinParams p;
  p.x = x; p.out = out; p.gamma = gamma; p.beta = beta; p.w = (const __bf16*)w_tiles; p.bias = bias_padded;
  p.res = res; p.res2 = res2; p.rs2 = res2_scale; p.xn = xn_out; p.ldxn = ldxn; p.M = M; p.ldx = ldx; p.ldo = ldo; p.ldr = ldr; p.ldr2 = ldr2;
  p.K = K; p.N = N; p.NT = n_tiles; p.act = act; p.eps = eps;
  FF_CHECK_ARG(!stats_out || (stat_lo >= 0 && stat_hi > stat_lo && stat_hi <= N && (((uintptr_t)stats_out) & 7) == 0), "ff_token_linear: bad statistics range");
  p.stats = stats_out; p.st_lo = stat_lo; p.st_hi = stat_hi; p.st_eps = stat_eps;
  p.x2 = nullptr; p.ldx2 = 0; p.cm = nullptr; p.gw1t = nullptr; p.gb1 = nullptr; p.gw2 = nullptr; p.gb2 = 0.f; p.wpi = 0;
  const bool vec4 = (N % 4 == 0) && (ldo % 4 == 0) && ((((uintptr_t)out) & 15) == 0) && (!res || (ldr % 4 == 0 && (((uintptr_t)res) & 15) == 0)) &&
           (!res2 || (ldr2 % 4 == 0 && (((uintptr_t)res2) & 15) == 0 && (((uintptr_t)res2_scale) & 15) == 0));
  const int ks = kpad / 16;
  const size_t lds = tl_lds(ks, n_tiles, 1);      // bias only
  FF_CHECK_ARG(lds <= FF_LDS_MAX, "ff_token_linear: N too large for the LDS image");
  FF_CHECK_ARG(act == ACT_NONE || act == ACT_GELU, "ff_token_linear: act must be none or gelu");
  const long long nblk = (M + 255) / 256;
  FF_CHECK_ARG(nblk < (1LL << 31), "ff_token_linear: grid too large");
#define TL_LAUNCH(A, KSV, V4, NTM)                                                                                          \
  do {                                                                                                                      \
    static ff_device_once once;                                                                                             \
    if (!ff_raise_lds(once, "ff_token_linear", FF_LDS_MAX, FF_LDS_SAY_ERR, &token_linear_kernel<A, KSV, V4, false, NTM>)) return FF_ERR_LAUNCH; \
    hipLaunchKernelGGL((token_linear_kernel<A, KSV, V4, false, NTM>), dim3((unsigned)nblk), dim3(512), lds, (hipStream_t)stream, p); \
  } while (0)
#define TL_LAUNCH_NT(A, KSV, V4) do { if (nterms == 3) TL_LAUNCH(A, KSV, V4, 3); else TL_LAUNCH(A, KSV, V4, 1); } while (0)
#define TL_LAUNCH_KS(A, V4) do { if (ks == 4) TL_LAUNCH_NT(A, 4, V4); else if (ks == 8) TL_LAUNCH_NT(A, 8, V4); else TL_LAUNCH_NT(A, 12, V4); } while (0)
  if (act == ACT_GELU) { if (vec4) TL_LAUNCH_KS(ACT_GELU, true); else TL_LAUNCH_KS(ACT_GELU, false); }
  else { if (vec4) TL_LAUNCH_KS(ACT_NONE, true); else TL_LAUNCH_KS(ACT_NONE, false); }
#undef TL_LAUNCH_KS
#undef TL_LAUNCH_NT
#undef TL_LAUNCH
  FF_LAUNCH_CHECK("ff_token_linear");
  return FF_OK;
}

// out16[token][n] = bf16( (LayerNorm?(x)[token] . W[n] + bias[n]) * col_scale[n] ), plain bf16 products: ff_token_linear's nterms == 1,
// ACT_NONE, VEC4 form with the fp32 result scaled per column and rounded on its way out.  The parameter list is ff_token_linear's (out in
// bf16 elements, col_scale [n_tiles*32] added); what this form does not have -- split products, an activation, residuals, the xn and
// statistics side outputs -- is refused in the first check.
extern "C" int ff_token_linear_rows16(const float* x, int ldx, void* out16, int ldo, long long M, int K, int kpad, int N, int n_tiles,
                                      const float* gamma, const float* beta, float eps, const void* w_tiles, const float* bias_padded,
                                      const float* col_scale, int act, const float* res, int ldr, const float* res2, int ldr2,
                                      const float* res2_scale, float* xn_out, int ldxn, float* stats_out, int stat_lo, int stat_hi,
                                      float stat_eps, int nterms, void* stream) {
  FF_CHECK_ARG(nterms == 1 && act == ACT_NONE && !res && !res2 && !res2_scale && !xn_out && !stats_out,
               "ff_token_linear_rows16: plain bf16 (nterms == 1), no activation, no res / res2 / xn_out / stats_out (got nterms=%d act=%d)", nterms, act);
  FF_CHECK_ARG(x && out16 && w_tiles && col_scale, "ff_token_linear_rows16: null pointer");
  FF_CHECK_ARG(M > 0 && K > 0 && K <= 192 && K % 4 == 0 && N > 0 && N % 4 == 0 && n_tiles * 32 >= N, "ff_token_linear_rows16: needs K <= 192, K and N multiples of 4, n_tiles*32 >= N");
  FF_CHECK_ARG(kpad == 64 || kpad == 128 || kpad == 192, "ff_token_linear_rows16: kpad must be 64, 128 or 192");
  FF_CHECK_ARG(kpad >= K, "ff_token_linear_rows16: kpad < K");
  FF_CHECK_ARG(ldx >= K && ldx % 4 == 0 && (((uintptr_t)x) & 15) == 0, "ff_token_linear_rows16: x rows must be 16-byte aligned");
  FF_CHECK_ARG(ldo >= N && ldo % 4 == 0 && (((uintptr_t)out16) & 7) == 0, "ff_token_linear_rows16: out rows must be 8-byte aligned (pitch in bf16 elements, a multiple of 4)");
  FF_CHECK_ARG((gamma == nullptr) == (beta == nullptr), "ff_token_linear_rows16: gamma/beta come together");
  FF_CHECK_ARG(((((uintptr_t)w_tiles) | ((uintptr_t)col_scale)) & 15) == 0 && (!gamma || ((((uintptr_t)gamma) & 15) == 0 && (((uintptr_t)beta) & 15) == 0)), "ff_token_linear_rows16: weights / col_scale / gamma / beta must be 16-byte aligned");
  TokenLinParams p;
  p.x = x; p.out = reinterpret_cast<float*>(out16); p.gamma = gamma; p.beta = beta; p.w = (const __bf16*)w_tiles; p.bias = bias_padded;
  p.res = nullptr; p.res2 = nullptr; p.rs2 = col_scale; p.xn = nullptr; p.ldxn = 0; p.M = M; p.ldx = ldx; p.ldo = ldo; p.ldr = 0; p.ldr2 = 0;
  p.K = K; p.N = N; p.NT = n_tiles; p.act = ACT_NONE; p.eps = eps;
  p.stats = nullptr; p.st_lo = 0; p.st_hi = 0; p.st_eps = 0.f;
  p.x2 = nullptr; p.ldx2 = 0; p.cm = nullptr; p.gw1t = nullptr; p.gb1 = nullptr; p.gw2 = nullptr; p.gb2 = 0.f; p.wpi = 0;
  const int ks = kpad / 16;
  const size_t lds = tl_lds(ks, n_tiles, 2);      // bias | column scale
  FF_CHECK_ARG(lds <= FF_LDS_MAX, "ff_token_linear_rows16: N too large for the LDS image");
  const long long nblk = (M + 255) / 256;
  FF_CHECK_ARG(nblk < (1LL << 31), "ff_token_linear_rows16: grid too large");
#define TL_LAUNCH16(KSV)                                                                                                    \
  do {                                                                                                                      \
    static ff_device_once once;                                                                                             \
    if (!ff_raise_lds(once, "ff_token_linear_rows16", FF_LDS_MAX, FF_LDS_SAY_ERR, &token_linear_rows16_kernel<ACT_NONE, KSV, true, false, 1>)) return FF_ERR_LAUNCH; \
    hipLaunchKernelGGL((token_linear_rows16_kernel<ACT_NONE, KSV, true, false, 1>), dim3((unsigned)nblk), dim3(512), lds, (hipStream_t)stream, p); \
  } while (0)
  if (ks == 4) TL_LAUNCH16(4); else if (ks == 8) TL_LAUNCH16(8); else TL_LAUNCH16(12);
#undef TL_LAUNCH16
  FF_LAUNCH_CHECK("ff_token_linear_rows16");
  return FF_OK;
}

// out = res + W . ( x * cm[channel] + x2 * sm[token] ) + b,  sm = sigmoid(gw2 . gelu(GW1 x + gb1) + gb2):  DAT's adaptive interaction
// (channel gate on one branch, spatial gate on the other, dat_arch.py:541-556 spatial blocks / :649-664 channel blocks) + the output
// projection (:559 / :666) + the block's residual in one launch.  gw1t: [192][12] floats = GW1 transposed and zero padded
// (11 hidden units, BatchNorm folded), gb1 / gw2: [12].
// The body of both entry points: B == 0 is ff_token_linear_gated (one cm vector, a grid of 256-token workgroups), B >= 1
// ff_token_linear_gated_images (cm [B][K], grid (rows_per_image / 256, B)).
static int token_linear_gated_launch(const char* who, const float* x, int ldx, const float* x2, int ldx2, const float* cm, int B, long long rows_per_image,
                                     const float* gw1t, const float* gb1, const float* gw2, float gb2, float* out, int ldo, long long M, int K, int N,
                                     int n_tiles, const void* w_tiles, const float* bias_padded, const float* res, int ldr, int nterms, void* stream) {
  FF_CHECK_ARG(nterms == 1 || nterms == 3, "%s: nterms must be 1 or 3", who);
  FF_CHECK_ARG(x && x2 && cm && gb1 && gw2 && out && w_tiles, "%s: null pointer", who);   /* gw1t is unused: GW1 travels as tile n_tiles of w_tiles */
  FF_CHECK_ARG(M > 0 && K > 0 && K <= 192 && K % 4 == 0 && N > 0 && N % 4 == 0 && n_tiles * 32 >= N, "%s: needs K <= 192, K and N multiples of 4", who);
  FF_CHECK_ARG(ldx >= K && ldx % 4 == 0 && ldx2 >= K && ldx2 % 4 == 0 && ldo >= N && ldo % 4 == 0 && (!res || (ldr >= N && ldr % 4 == 0)), "%s: rows must be 16-byte aligned", who);
  FF_CHECK_ARG(((((uintptr_t)x) | ((uintptr_t)x2) | ((uintptr_t)cm) | ((uintptr_t)out) | ((uintptr_t)w_tiles) | ((uintptr_t)res)) & 15) == 0, "%s: 16-byte alignment", who);
  const long long wpi = B ? rows_per_image / 256 : 0, nblk = B ? wpi : (M + 255) / 256;
  FF_CHECK_ARG(nblk < (1LL << 31), "%s: grid too large", who);
  TokenLinParams p{};
  p.x = x; p.out = out; p.w = (const __bf16*)w_tiles; p.bias = bias_padded; p.res = res; p.M = M; p.ldx = ldx; p.ldo = ldo; p.ldr = ldr;
  p.K = K; p.N = N; p.NT = n_tiles; p.act = ACT_NONE;
  p.x2 = x2; p.ldx2 = ldx2; p.cm = cm; p.gw1t = gw1t; p.gb1 = gb1; p.gw2 = gw2; p.gb2 = gb2; p.wpi = (int)wpi;
  const size_t lds = tl_lds(12, n_tiles, 1);      // the gated kernels are the KS = 12 instantiations; bias only
  FF_CHECK_ARG(lds <= FF_LDS_MAX, "%s: N too large for the LDS image", who);
  static ff_device_once once[2];
  if (!(!B ? ff_raise_lds(once[0], who, FF_LDS_MAX, FF_LDS_SAY_ERR, &token_linear_kernel<ACT_NONE, 12, true, true, 3>, &token_linear_kernel<ACT_NONE, 12, true, true, 1>)
           : ff_raise_lds(once[1], who, FF_LDS_MAX, FF_LDS_SAY_ERR, &token_linear_images_kernel<ACT_NONE, 12, true, true, 3>, &token_linear_images_kernel<ACT_NONE, 12, true, true, 1>)))
    return FF_ERR_LAUNCH;
  const dim3 grid((unsigned)nblk, B ? (unsigned)B : 1u);
  if (!B) {
    if (nterms == 3) hipLaunchKernelGGL((token_linear_kernel<ACT_NONE, 12, true, true, 3>), grid, dim3(512), lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((token_linear_kernel<ACT_NONE, 12, true, true, 1>), grid, dim3(512), lds, (hipStream_t)stream, p);
  } else {
    if (nterms == 3) hipLaunchKernelGGL((token_linear_images_kernel<ACT_NONE, 12, true, true, 3>), grid, dim3(512), lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((token_linear_images_kernel<ACT_NONE, 12, true, true, 1>), grid, dim3(512), lds, (hipStream_t)stream, p);
  }
  FF_LAUNCH_CHECK(who);
  return FF_OK;
}

extern "C" int ff_token_linear_gated(const float* x, int ldx, const float* x2, int ldx2, const float* cm, const float* gw1t,
                                     const float* gb1, const float* gw2, float gb2, float* out, int ldo, long long M, int K, int N,
                                     int n_tiles, const void* w_tiles, const float* bias_padded, const float* res, int ldr, int nterms,
                                     void* stream) {
  return token_linear_gated_launch("ff_token_linear_gated", x, ldx, x2, ldx2, cm, 0, 0, gw1t, gb1, gw2, gb2, out, ldo, M, K, N, n_tiles, w_tiles, bias_padded, res, ldr, nterms, stream);
}

// ff_token_linear_gated over B images of rows_per_image tokens each, with one channel gate per image: cm is [B][K] (contiguous rows).  A
// workgroup owns 256 tokens, so rows_per_image must be a multiple of 256 -- no workgroup straddles two images -- and M == B * rows_per_image.
// Every row comes out with the bits of ff_token_linear_gated on its image alone with cm[b].
extern "C" int ff_token_linear_gated_images(const float* x, int ldx, const float* x2, int ldx2, const float* cm, int B, long long rows_per_image,
                                            const float* gb1, const float* gw2, float gb2, float* out, int ldo, long long M, int K, int N,
                                            int n_tiles, const void* w_tiles, const float* bias_padded, const float* res, int ldr, int nterms,
                                            void* stream) {
  FF_CHECK_ARG(B > 0 && B <= 65535 && rows_per_image > 0 && rows_per_image % 256 == 0 && M == (long long)B * rows_per_image,
               "ff_token_linear_gated_images: rows_per_image must be a positive multiple of 256 and M == B * rows_per_image (1 <= B <= 65535; got B=%d rows_per_image=%lld M=%lld)",
               B, rows_per_image, M);
  return token_linear_gated_launch("ff_token_linear_gated_images", x, ldx, x2, ldx2, cm, B, rows_per_image, nullptr, gb1, gw2, gb2, out, ldo, M, K, N, n_tiles, w_tiles, bias_padded, res, ldr, nterms, stream);
}
