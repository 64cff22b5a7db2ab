// Implicit-GEMM convolution / GEMM on the bf16 matrix cores with fp32-grade accuracy by operand
// splitting ("bf16x3"):  a = a_hi + a_lo (+ O(2^-16 |a|)),  both halves bf16, so
//     a*w  ~=  a_hi*w_hi + a_lo*w_hi + a_hi*w_lo          (the dropped a_lo*w_lo term is O(2^-16))
// Each term is one v_mfma_f32_32x32x16_bf16 into the SAME fp32 accumulator: 3 MFMAs at 16x the fp32
// MFMA rate = 5.3x the fp32-MFMA ceiling of conv_gemm.hip at the same results to ~1e-5 relative.
// NTERMS = 1 (plain bf16) and 2 (fp32-accurate activations x bf16 weights) are the cheaper modes.
//
// Same contract / epilogue as conv_gemm.hip.  Differences:
//   - weights arrive pre-split by ff_split_bf16 as two bf16 planes w_hi/w_lo [Cout][Kp], Kp = K rounded up
//     to 32 (zero filled), so the B tile is a straight 16-byte copy with no K tail;
//   - activations are split on the fly in the staging path (v_cvt_pk_bf16_f32), once per element per
//     workgroup, and stored to LDS as [row][hi k0..31 | lo k0..31] (128 B + 16 B pad = 36 dwords:
//     36 = 4*9 puts the 16 rows of a ds_read_b128 lane group on 16 distinct 4-bank slots);
//   - BK = 32: two k-steps of the 32x32x16 MFMA per chunk; a lane's operand is one ds_read_b128
//     (8 consecutive k of its row) per plane and k-step;
//   - K is laid out per filter tap with the tap's Cin padded to Cp = ceil32(Cin) when Cin >= 32 ("TAP" mode:
//     a chunk never straddles taps, so (tap, ci0) are wave-uniform scalars and the per-thread gather needs no
//     division); small-Cin convolutions (3, 9, 27 ... input channels) keep the flat k = (tap, ci) order;
//   - tiles: 256x192 with 8 waves (64x96 per wave, 36 MFMAs per chunk and wave) for the 180/360/540/720-wide
//     transformer layers (65536 tokens -> exactly 256 workgroups per 192 columns: one per CU, no tail),
//     128x128 / 128x64 / 256x32 with 4 waves elsewhere.
#include "ff_common.h"

struct ConvBfParams {
  const float* in;
  const __bf16* w_hi;
  const __bf16* w_lo;
  const float* bias;
  const float* mul;
  const float* res;
  const float* kmul;   // optional [Cin] scale of the INPUT channels (1x1 only): out = W (kmul * a) -- NAFNet's conv3(x * sca)
  float* out;
  int B, H, W, Cin, ldi;
  int Ho, Wo, Cout, ldo, ldr;
  int KH, KW, sy, sx, py, px;
  int K, Kp, M;
  int Cp;          // TAP mode: per-tap padded Cin (multiple of 32); 0 = flat k order
  int act;
  float alpha;
  int shuffle;
  int vec_out;     // 16-byte epilogue: no shuffle, Cout % 4 == 0, 16-byte aligned out / res rows
  int gate;        // shuffle == 1: SimpleGate in the epilogue, out[m][j] = y[m][2j] * y[m][2j+1] (Cout / 2 channels out)
};

#define CIG_KERNEL conv_igemm_bf16_kernel
#define CIG_KMUL_IMAGES 0
#define CIG_W_IMAGES 0
#include "conv_igemm_bf16_kernel.inc"
#undef CIG_KERNEL
#undef CIG_KMUL_IMAGES
#define CIG_KERNEL conv_igemm_bf16_kmimg_kernel
#define CIG_KMUL_IMAGES 1
#include "conv_igemm_bf16_kernel.inc"
#undef CIG_KERNEL
#undef CIG_KMUL_IMAGES
#undef CIG_W_IMAGES
#define CIG_KERNEL conv_igemm_bf16_wimg_kernel
#define CIG_KMUL_IMAGES 0
#define CIG_W_IMAGES 1
#include "conv_igemm_bf16_kernel.inc"
#undef CIG_KERNEL
#undef CIG_KMUL_IMAGES
#undef CIG_W_IMAGES

// The two per-image forms of the 1x1 GEMM share one launcher and one dispatcher.  WIMG picks the kernel and the entry point's name:
// per-image weight planes (ff_conv2d_bf16s_wimages) or per-image kmul rows (ff_conv2d_bf16s_kmul_images).
template <bool WIMG>
static const char* bf_images_who() { return WIMG ? "ff_conv2d_bf16s_wimages" : "ff_conv2d_bf16s_kmul_images"; }

template <bool WIMG, int BM, int BN, int WM, int WN, int NT>
static int launch_bf_images(const ConvBfParams& p, hipStream_t st) {
  const char* const who = bf_images_who<WIMG>();
  const int mt = ff_cdiv(p.M, BM), nt = ff_cdiv(p.Cout, BN);
  constexpr size_t lds = gemm_lds(BM, BN, cig_rowb(32));
  static_assert(lds <= FF_LDS_MAX, "LDS budget");
  static_assert(!WIMG || 256 % BM == 0, "an m-tile must not straddle two images of a multiple of 256 rows");
  void (*kernel)(ConvBfParams);
  if constexpr (WIMG) kernel = &conv_igemm_bf16_wimg_kernel<BM, BN, WM, WN, true, NT, 32>;
  else kernel = &conv_igemm_bf16_kmimg_kernel<BM, BN, WM, WN, true, NT, 32>;
  static ff_device_once once;
  if (lds > FF_LDS_DEFAULT_MAX && !ff_raise_lds(once, who, lds, FF_LDS_SAY_SIZE | FF_LDS_SAY_ERR, kernel)) return FF_ERR_LAUNCH;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(mt * nt)), dim3(WM * WN * 64), lds, st, p);
  FF_LAUNCH_CHECK(who);
  return FF_OK;
}

// the configurations ff_conv2d_bf16s_tile can name for a 1x1 with 16-byte rows
template <bool WIMG, int NT>
static int dispatch_bf_images(const ConvBfParams& p, int cfg, hipStream_t st) {
  switch (cfg) {
    case 3: return launch_bf_images<WIMG, 256, 32, 4, 1, NT>(p, st);
    case 4: return launch_bf_images<WIMG, 256, 192, 4, 2, NT>(p, st);
    case 5: return launch_bf_images<WIMG, 128, 128, 2, 4, NT>(p, st);
    case 7: return launch_bf_images<WIMG, 128, 64, 4, 2, NT>(p, st);
    default: ff_set_error("%s: tile_hint %d is not one of 3, 4, 5, 7", bf_images_who<WIMG>(), cfg); return FF_ERR_ARG;
  }
}

template <int BM, int BN, int WM, int WN, int NT, int BKB = 32>
static int launch_bf(const ConvBfParams& p, bool vec4, hipStream_t st) {
  const int mt = ff_cdiv(p.M, BM), nt = ff_cdiv(p.Cout, BN);
  constexpr size_t lds = gemm_lds(BM, BN, cig_rowb(BKB));
  static_assert(lds <= FF_LDS_MAX, "LDS budget (staging ring; the epilogue patches reuse it: asserted in the kernel)");
  dim3 grid((unsigned)(mt * nt)), block(WM * WN * 64);
  static ff_device_once once[2];       // [vec4]
  if (lds > FF_LDS_DEFAULT_MAX && !(vec4 ? ff_raise_lds(once[1], "ff_conv2d_bf16s", lds, FF_LDS_SAY_SIZE | FF_LDS_SAY_ERR, &conv_igemm_bf16_kernel<BM, BN, WM, WN, true, NT, BKB>)
                                : ff_raise_lds(once[0], "ff_conv2d_bf16s", lds, FF_LDS_SAY_SIZE | FF_LDS_SAY_ERR, &conv_igemm_bf16_kernel<BM, BN, WM, WN, false, NT, BKB>)))
    return FF_ERR_LAUNCH;
  if (vec4)
    hipLaunchKernelGGL((conv_igemm_bf16_kernel<BM, BN, WM, WN, true, NT, BKB>), grid, block, lds, st, p);
  else
    hipLaunchKernelGGL((conv_igemm_bf16_kernel<BM, BN, WM, WN, false, NT, BKB>), grid, block, lds, st, p);
  FF_LAUNCH_CHECK("ff_conv2d_bf16s");
  return FF_OK;
}

template <int NT>
static int dispatch_bf(const ConvBfParams& p, bool vec4, int cfg, hipStream_t st) {
  switch (cfg) {
    case 1: return launch_bf<128, 128, 2, 2, NT>(p, vec4, st);
    case 2: return launch_bf<128, 64, 2, 2, NT>(p, vec4, st);
    case 3: return launch_bf<256, 32, 4, 1, NT>(p, vec4, st);
    case 4: return launch_bf<256, 192, 4, 2, NT>(p, vec4, st);
    case 5: return launch_bf<128, 128, 2, 4, NT>(p, vec4, st);      // 8 waves (two per SIMD), 64x32 per wave
    case 6: return launch_bf<256, 128, 4, 2, NT>(p, vec4, st);      // 8 waves, 64x64 per wave
    case 7: return launch_bf<128, 64, 4, 2, NT>(p, vec4, st);       // 8 waves, 32x32 per wave
    // 64-deep chunks (Kp and the per-tap Cp must be multiples of 64; checked by the caller below)
    case 8: return launch_bf<128, 128, 2, 4, NT, 64>(p, vec4, st);
    case 9: return launch_bf<128, 64, 4, 2, NT, 64>(p, vec4, st);
    default: ff_set_error("ff_conv2d_bf16s: bad tile_hint %d", cfg); return FF_ERR_ARG;
  }
}

// The tile configuration ff_conv2d_bf16s picks for tile_hint <= 0, from M = B * Ho * Wo output rows, Cout, K = KH * KW * Cin and whether the
// input rows take 16-byte loads.  Exported so that a caller that batches independent images can pass the configuration ONE image would get
// as its tile_hint (isr2_amd.ops.conv2d(per_image=True)): batched and single-image launches then take the same kernel form.
extern "C" int ff_conv2d_bf16s_tile(long long M, int Cout, int K, int vec4) {
  // measured on MI355X (profiles/r01_gemm_shapes_bf16x3_v2.txt): 128x128 tiles win whenever N pads well or K is long
  const int r192 = Cout % 192, r128 = Cout % 128;
  // r2 (profiles/r02_gemm_shapes_8wave.txt): the 8-wave forms of the 128-row tiles (two waves per SIMD: one wave's operand
  // reads and global-load waits hide behind the other's MFMAs) beat the 4-wave forms on every 1x1 shape: cfg 5 replaces 1, 7 replaces 2
  if (Cout <= 32) return 3;
  if (Cout <= 64) return 7;
  if (r128 == 0) return 5;
  // measured (profiles/r01_gemm_shapes_bf16x3_v3.txt): 256x192 wins for N <= 192 or long K; 128x128 for wide N at K = 180
  if (vec4 && M >= 256 * 64 && (r192 == 0 || r192 > 128) && (Cout <= 192 || K >= 320)) return 4;
  if (Cout > 256 || (Cout > 128 && K >= 512)) return 5;
  return 7;
}

extern "C" int ff_conv2d_bf16s(const float* in, const void* w_hi, const void* w_lo, int Kp, int Cp, const float* bias,
                               const float* mul, const float* res, float* out, int B, int H, int W, int Cin, int ldi,
                               int Ho, int Wo, int Cout, int ldo, int ldr, int KH, int KW, int sy, int sx, int py, int px,
                               int act, float alpha, int shuffle, int nterms, int tile_hint, const float* kmul, void* stream) {
  FF_CHECK_ARG(in && w_hi && out, "ff_conv2d_bf16s: null pointer");
  FF_CHECK_ARG(!kmul || (KH == 1 && KW == 1 && Cin % 4 == 0 && (((uintptr_t)kmul) & 15) == 0), "ff_conv2d_bf16s: kmul needs a 1x1 kernel, Cin %% 4 == 0 and a 16-byte aligned vector");
  FF_CHECK_ARG(nterms >= 1 && nterms <= 3 && (nterms < 3 || w_lo), "ff_conv2d_bf16s: nterms must be 1..3 (3 needs w_lo)");
  FF_CHECK_ARG(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Ho > 0 && Wo > 0, "ff_conv2d_bf16s: bad dims");
  FF_CHECK_ARG(ldi >= Cin, "ff_conv2d_bf16s: ldi %d < Cin %d", ldi, Cin);
  FF_CHECK_ARG(KH > 0 && KW > 0 && sy > 0 && sx > 0 && py >= 0 && px >= 0, "ff_conv2d_bf16s: bad kernel geometry");
  FF_CHECK_ARG(Kp % 32 == 0 && Kp >= KH * KW * Cin, "ff_conv2d_bf16s: Kp must be K rounded up to 32");
  FF_CHECK_ARG(Cp == 0 || (Cp % 32 == 0 && Cp >= Cin && Kp == KH * KW * Cp), "ff_conv2d_bf16s: TAP layout needs Kp == taps * Cp, Cp = ceil32(Cin)");
  FF_CHECK_ARG((((uintptr_t)w_hi) & 15) == 0 && (!w_lo || (((uintptr_t)w_lo) & 15) == 0), "ff_conv2d_bf16s: weight planes must be 16-byte aligned");
  FF_CHECK_ARG(shuffle == 0 || shuffle == 1 || shuffle == 2, "ff_conv2d_bf16s: shuffle must be 0, 1 (SimpleGate pair product) or 2 (PixelShuffle)");
  FF_CHECK_ARG(shuffle != 2 || Cout % 4 == 0, "ff_conv2d_bf16s: shuffle needs Cout %% 4 == 0");
  FF_CHECK_ARG(shuffle != 1 || (Cout % 8 == 0 && !res && !mul && act == 0 && alpha == 1.f && ldo % 4 == 0 && (((uintptr_t)out) & 15) == 0),
               "ff_conv2d_bf16s: the pair-product epilogue needs Cout %% 8 == 0, no residual / scale / activation and 16-byte aligned output rows");
  FF_CHECK_ARG(ldo >= (shuffle == 2 ? Cout / 4 : shuffle == 1 ? Cout / 2 : Cout), "ff_conv2d_bf16s: ldo too small");
  FF_CHECK_ARG(!res || ldr >= (shuffle ? Cout / 4 : Cout), "ff_conv2d_bf16s: ldr too small");
  FF_CHECK_ARG((long long)B * Ho * Wo < (1LL << 31), "ff_conv2d_bf16s: M overflows int");
  ConvBfParams p;
  p.in = in; p.w_hi = (const __bf16*)w_hi; p.w_lo = (const __bf16*)w_lo; p.bias = bias; p.mul = mul; p.res = res; p.out = out;
  p.kmul = kmul; p.gate = shuffle == 1 ? 1 : 0;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.ldi = ldi;
  p.Ho = Ho; p.Wo = Wo; p.Cout = Cout; p.ldo = ldo; p.ldr = ldr;
  p.KH = KH; p.KW = KW; p.sy = sy; p.sx = sx; p.py = py; p.px = px;
  p.K = KH * KW * Cin; p.Kp = Kp; p.Cp = Cp; p.M = B * Ho * Wo;
  p.act = act; p.alpha = alpha; p.shuffle = shuffle;
  p.vec_out = shuffle == 0 && Cout % 4 == 0 && ldo % 4 == 0 && (((uintptr_t)out) & 15) == 0 &&
              (!res || (ldr % 4 == 0 && (((uintptr_t)res) & 15) == 0));
  const bool vec4 = (Cin % 4 == 0) && (ldi % 4 == 0) && (((uintptr_t)in & 15) == 0);
  FF_CHECK_ARG(Cp == 0 || vec4, "ff_conv2d_bf16s: TAP layout needs Cin %% 4 == 0 and 16-byte aligned rows");
  FF_CHECK_ARG(!kmul || vec4, "ff_conv2d_bf16s: kmul needs 16-byte aligned input rows");
  hipStream_t st = (hipStream_t)stream;
  int cfg = tile_hint;
  if (cfg <= 0) cfg = ff_conv2d_bf16s_tile(p.M, Cout, p.K, vec4 ? 1 : 0);
  const bool k64 = Kp % 64 == 0 && (Cp == 0 || Cp % 64 == 0) && vec4;
  if (cfg >= 8 && !k64) cfg = cfg == 8 ? 5 : 7;
  switch (nterms) {
    case 1: return dispatch_bf<1>(p, vec4, cfg, st);
    case 2: return dispatch_bf<2>(p, vec4, cfg, st);
    default: return dispatch_bf<3>(p, vec4, cfg, st);
  }
}

// The body of the two per-image 1x1 entry points below, after their own checks of B, rows_per_image and M: the checks they share (the two
// whose wording differs pick it by form), the params fill and the dispatch.  kmul is [B][Cin] (WIMG: nullptr), w_hi / w_lo [B][Cout][Kp] if WIMG.
template <bool WIMG>
static int conv2d_bf16s_images_launch(const float* in, int ldi, const void* w_hi, const void* w_lo, int Kp, int Cp, const float* kmul, int B,
                                      int rows_per_image, const float* bias, const float* mul, const float* res, int ldr, float* out, int ldo,
                                      long long M, int Cin, int Cout, int nterms, int tile_hint, void* stream) {
  const char* const who = bf_images_who<WIMG>();
  FF_CHECK_ARG(in && w_hi && out && (WIMG || kmul), "%s: null pointer", who);
  FF_CHECK_ARG(nterms >= 1 && nterms <= 3 && (nterms < 3 || w_lo), "%s: nterms must be 1..3 (3 needs w_lo)", who);
  FF_CHECK_ARG(Cin > 0 && Cout > 0 && Cin % 4 == 0 && ldi >= Cin && ldi % 4 == 0 && (((uintptr_t)in) & 15) == 0 && (((uintptr_t)kmul) & 15) == 0,
               WIMG ? "%s: needs Cin %% 4 == 0 and 16-byte aligned input rows (ldi %% 4 == 0)"
                    : "%s: needs Cin %% 4 == 0, 16-byte aligned input rows (ldi %% 4 == 0) and kmul", who);
  FF_CHECK_ARG(Kp % 32 == 0 && Kp >= Cin && (Cp == 0 || (Cp % 32 == 0 && Cp >= Cin && Kp == Cp)), "%s: Kp must be Cin rounded up to 32 (TAP layout: Kp == Cp)", who);
  FF_CHECK_ARG((((uintptr_t)w_hi) & 15) == 0 && (!w_lo || (((uintptr_t)w_lo) & 15) == 0) && (!WIMG || ((long long)Cout * Kp) % 8 == 0),
               WIMG ? "%s: every image's weight planes must be 16-byte aligned" : "%s: weight planes must be 16-byte aligned", who);
  FF_CHECK_ARG(Cout % 4 == 0 && ldo >= Cout && ldo % 4 == 0 && (((uintptr_t)out) & 15) == 0 && (!res || (ldr >= Cout && ldr % 4 == 0 && (((uintptr_t)res) & 15) == 0)),
               "%s: needs Cout %% 4 == 0 and 16-byte aligned output / residual rows", who);
  ConvBfParams p{};
  p.in = in; p.w_hi = (const __bf16*)w_hi; p.w_lo = (const __bf16*)w_lo; p.bias = bias; p.mul = mul; p.res = res; p.out = out;
  p.kmul = kmul;
  p.B = B; p.H = 1; p.W = rows_per_image; p.Cin = Cin; p.ldi = ldi;
  p.Ho = 1; p.Wo = rows_per_image; p.Cout = Cout; p.ldo = ldo; p.ldr = ldr;
  p.KH = 1; p.KW = 1; p.sy = 1; p.sx = 1;
  p.K = Cin; p.Kp = Kp; p.Cp = Cp; p.M = (int)M;
  p.alpha = 1.f; p.vec_out = 1;
  hipStream_t st = (hipStream_t)stream;
  int cfg = tile_hint;
  if (cfg <= 0) cfg = ff_conv2d_bf16s_tile(rows_per_image, Cout, Cin, 1);
  switch (nterms) {
    case 1: return dispatch_bf_images<WIMG, 1>(p, cfg, st);
    case 2: return dispatch_bf_images<WIMG, 2>(p, cfg, st);
    default: return dispatch_bf_images<WIMG, 3>(p, cfg, st);
  }
}

// conv3 of B independent images in one launch (1x1): in is fp32 [M][ldi] rows, M == B * rows_per_image, kmul is [B][Cin] and row m is
// scaled by kmul[m / rows_per_image] before the split.  Epilogue: (acc + bias) * mul + res, the 16-byte form.  Every row is bit-equal to
// ff_conv2d_bf16s(1x1, kmul = kmul[b]) on its image alone; tile_hint <= 0 takes ff_conv2d_bf16s_tile of ONE image's rows.
extern "C" int ff_conv2d_bf16s_kmul_images(const float* in, int ldi, const void* w_hi, const void* w_lo, int Kp, int Cp, const float* kmul,
                                           int B, int rows_per_image, const float* bias, const float* mul, const float* res, int ldr,
                                           float* out, int ldo, long long M, int Cin, int Cout, int nterms, int tile_hint, void* stream) {
  FF_CHECK_ARG(B >= 1 && rows_per_image >= 1 && M == (long long)B * rows_per_image && M < (1LL << 31),
               "ff_conv2d_bf16s_kmul_images: M must be B * rows_per_image and below 2^31 (got M=%lld B=%d rows_per_image=%d)", M, B, rows_per_image);
  return conv2d_bf16s_images_launch<false>(in, ldi, w_hi, w_lo, Kp, Cp, kmul, B, rows_per_image, bias, mul, res, ldr, out, ldo, M, Cin, Cout, nterms, tile_hint, stream);
}

// A 1x1 GEMM whose rows are B equal groups, each multiplied by its OWN weight planes: in is fp32 [M][ldi] rows, M == B * rows_per_image,
// w_hi / w_lo are [B][Cout][Kp] (ff_split_bf16 called once on the [B * Cout][Cin] matrix: its rows are independent) and row m takes the planes
// of image m / rows_per_image.  rows_per_image must be a multiple of 256, the tallest tile, so no m-tile straddles two images.  The K order
// and the epilogue ((acc + bias) * mul + res, the 16-byte form) are those of ff_conv2d_bf16s: every row is bit-equal to ff_conv2d_bf16s(1x1) on
// its image alone with its planes; tile_hint <= 0 takes ff_conv2d_bf16s_tile of ONE image's rows.  DAT's att = v . wbd^T (dat_arch.py:647).
extern "C" int ff_conv2d_bf16s_wimages(const float* in, int ldi, const void* w_hi, const void* w_lo, int Kp, int Cp, int B, int rows_per_image,
                                       const float* bias, const float* mul, const float* res, int ldr, float* out, int ldo, long long M,
                                       int Cin, int Cout, int nterms, int tile_hint, void* stream) {
  FF_CHECK_ARG(B >= 1 && rows_per_image >= 1 && rows_per_image % 256 == 0 && M == (long long)B * rows_per_image && M < (1LL << 31),
               "ff_conv2d_bf16s_wimages: rows_per_image must be a positive multiple of 256, M == B * rows_per_image and below 2^31 (got M=%lld B=%d rows_per_image=%d)",
               M, B, rows_per_image);
  return conv2d_bf16s_images_launch<true>(in, ldi, w_hi, w_lo, Kp, Cp, nullptr, B, rows_per_image, bias, mul, res, ldr, out, ldo, M, Cin, Cout, nterms, tile_hint, stream);
}

// fp32 [N][K] -> bf16 planes hi/lo [N][Kp], zero filled; lo may be NULL.
// Cp == 0: flat, Kp = ceil32(K).  Cp > 0 (TAP layout): K = taps*Cin, column tap*Cp + ci holds w[n][tap*Cin + ci].
__global__ __launch_bounds__(256) void split_bf16_kernel(const float* __restrict__ w, int N, int K, int Kp, int Cin, int Cp,
                                                         __bf16* __restrict__ hi, __bf16* __restrict__ lo) {
  const long long total = (long long)N * Kp;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int kp = (int)(i % Kp);
    const long long n = i / Kp;
    int k = kp;
    bool ok = kp < K;
    if (Cp > 0) { const int tap = kp / Cp, ci = kp - tap * Cp; ok = ci < Cin; k = tap * Cin + ci; }
    const float f = ok ? w[n * K + k] : 0.f;
    const __bf16 h = (__bf16)f;
    hi[i] = h;
    if (lo) lo[i] = (__bf16)(f - (float)h);
  }
}

extern "C" int ff_split_bf16(const float* w, int N, int K, int Kp, int Cin, int Cp, void* hi, void* lo, void* stream) {
  FF_CHECK_ARG(w && hi && N > 0 && K > 0 && Kp % 32 == 0 && Kp >= K, "ff_split_bf16: bad args");
  FF_CHECK_ARG(Cp == 0 || (Cin > 0 && K % Cin == 0 && Cp % 32 == 0 && Cp >= Cin && Kp == (K / Cin) * Cp), "ff_split_bf16: bad TAP layout");
  long long nb = ((long long)N * Kp + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, w, N, K, Kp, Cin, Cp, (__bf16*)hi, (__bf16*)lo);
  FF_LAUNCH_CHECK("ff_split_bf16");
  return FF_OK;
}
