// NAFBlock tail in one launch, plain bf16 (one MFMA term), C = 64 / 128 (nafnet_arch.py:118-131):
//     y   = x + beta  * (W3 (g * sca) + b3)                                  (conv3 on the SCA-scaled gate, first residual)
//     out = y + gamma * (W5 SimpleGate(W4 LayerNorm2d(y) + b4) + b5)         (the gated FFN, second residual)
// Replaces ff_conv2d_bf16s(kmul = sca, res = x, mul = beta) + ff_naf_ffn(nterms = 1) and the round trip of y through HBM between
// them: g and x in, out out -- 805 MB instead of 1 342 MB at c = 64 / 1024 x 1024, 403 instead of 671 MB at c = 128 / 512 x 512.
//
// Dataflow.  Lane = token, wave = 32 tokens (as naf_ffn_kernel).  In plain bf16 there are no lo planes, so ALL weights
// (W3, W4, W5: 4 C^2 bf16 = 32 / 128 KB) stay in LDS for the life of the workgroup, stored in MFMA A-fragment order
// ([fragment][lane][8 bf16]: every operand read is one conflict-free ds_read_b128, no row padding), and the workgroups are
// persistent: 2 per CU (c = 64, 4 waves) or 1 per CU (c = 128, 4 waves: one per SIMD, with a 4.5 KB row-gather patch each next to the 128 KB of weights)
// stride over the token tiles, so the weight image is fetched once per workgroup and no barrier follows the first one.
// A wave brings the g and x rows of its NEXT tile into registers while it computes the current one (the only HBM latency
// left exposed is the first tile's).
//
// Rounding contract: bit-equal to the two launches it replaces.
//   1. A operand of conv3 = bf16(g * sca[k]), product in fp32; K accumulated in ascending 16-wide MFMA steps from zero
//      (conv_gemm_bf16.hip: load_chunk / store_chunk, one accumulator per output tile).
//   2. t = (acc + b3) * beta rounded to fp32, THEN y = t + x: the 16-byte epilogue of conv_igemm_bf16_kernel stores t to LDS
//      before it adds the residual, so there is no fused multiply-add across the two.  Here every t passes through
//      v_permlane32_swap (below), which the compiler cannot contract through either.
//   3. The conv3 accumulator holds, for token l31, channels 8q + 4hh + e of each 32-channel tile; naf_ffn_kernel's row gather
//      holds channels 16st + 8hh + j.  The two differ by an exchange between the wave's halves only: one v_permlane32_swap per
//      register pair puts y into exactly the gather's layout, so the LayerNorm sums run in naf_ffn_kernel's order and its
//      body is reused unchanged from there.
//   4. y never reaches HBM: it stays in registers and is the final residual (transposed through the wave's LDS patch next
//      to the accumulator tile, the same expression as naf_ffn_kernel's epilogue).
//
// Resource usage: the table at the launcher.  Measured (MI355X, HIP events, 20 back-to-back launches): c = 64, M = 1 048 576:
// 160 us (5.0 TB/s) against 324 us for the two launches; c = 128, M = 262 144: 115-124 us (3.3-3.5 TB/s) against 179-184 us.
#include "ff_common.h"

struct NafTailParams {
  const float* g; const float* x; float* out;
  const __bf16* w;        // prep.pack_naf_tail: [W3 | W4 | W5] fragments, 4 C^2 bf16
  const float* sca;       // [C] channel attention (scale of conv3's input channels)
  const float* b3;        // [C]
  const float* beta;      // [C] NAFBlock beta
  const float* gamma_ln; const float* beta_ln;
  const float* b4;        // [2C]
  const float* b5;        // [C]
  const float* oscale;    // [C] NAFBlock gamma
  long long M;
  int ldg, ldx, ldo;
  int ntiles;
  float eps;
  int rpi, nimg;          // naf_tail_images_kernel: rows per image (a multiple of 32: a wave's 32 rows are one image's), images; sca is [nimg][C]
};

#define NAF_TAIL_KERNEL naf_tail_kernel
#define NAF_TAIL_IMG 0
#include "naf_tail_kernel.inc"
#undef NAF_TAIL_KERNEL
#undef NAF_TAIL_IMG
#define NAF_TAIL_KERNEL naf_tail_images_kernel       // rows of B images, sca [B][C] (ff_naf_tail_images)
#define NAF_TAIL_IMG 1
#include "naf_tail_kernel.inc"
#undef NAF_TAIL_KERNEL
#undef NAF_TAIL_IMG

// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage:
//   kernel            VGPRs  AGPRs  scratch  LDS (dynamic)  waves/SIMD  workgroups/CU
//   naf_tail<4, 4>    252    0      0        69 888 B       2           2  (c = 64: 8 waves per CU)
//   naf_tail<8, 4>    256    202    0        154 112 B      1           1  (c = 128: 4 waves per CU)
//   naf_tail_images<4, 4>  256  0    0        70 912 B       2           2  (+ NW * C floats: one sca slot per wave)
//   naf_tail_images<8, 4>  256  208  0        156 160 B      1           1
template <int KS, int NW, int WGPC, bool IMG = false>
static int launch_naf_tail(NafTailParams& p, hipStream_t st) {
  constexpr size_t lds = ntl_lds(KS, NW, IMG);
  static_assert(lds <= FF_LDS_MAX, "LDS budget");
  static ff_device_once once;
  if (!(IMG ? ff_raise_lds(once, "ff_naf_tail", lds, FF_LDS_SAY_ERR, &naf_tail_images_kernel<KS, NW>)
            : ff_raise_lds(once, "ff_naf_tail", lds, FF_LDS_SAY_ERR, &naf_tail_kernel<KS, NW>))) return FF_ERR_LAUNCH;
  const long long ntiles = (p.M + NW * 32 - 1) / (NW * 32);
  if (ntiles >= (1LL << 31)) { ff_set_error("ff_naf_tail: too many rows"); return FF_ERR_ARG; }
  p.ntiles = (int)ntiles;
  const long long nblk = ntiles < 256 * WGPC ? ntiles : 256 * WGPC;      // persistent: WGPC workgroups per CU stride over the tiles
  if (IMG)
    hipLaunchKernelGGL((naf_tail_images_kernel<KS, NW>), dim3((unsigned)nblk), dim3(NW * 64), lds, st, p);
  else
    hipLaunchKernelGGL((naf_tail_kernel<KS, NW>), dim3((unsigned)nblk), dim3(NW * 64), lds, st, p);
  FF_LAUNCH_CHECK("ff_naf_tail");
  return FF_OK;
}

// The body of both entry points: B == 0 is ff_naf_tail (one sca vector for all rows), B >= 1 ff_naf_tail_images (sca [B][C]).
static int naf_tail_launch(const char* who, const float* g, int ldg, const float* x, int ldx, float* out, int ldo, long long M, int C,
                           const float* sca, int B, int rows_per_image, const float* b3, const float* beta, const float* gamma_ln,
                           const float* beta_ln, float eps, const void* w_frags, const float* b4, const float* b5, const float* out_scale,
                           void* stream) {
  FF_CHECK_ARG(g && x && out && sca && b3 && beta && gamma_ln && beta_ln && w_frags && b4 && b5 && out_scale, "%s: null pointer", who);
  FF_CHECK_ARG(M > 0 && (C == 64 || C == 128), "%s: C must be 64 or 128", who);
  FF_CHECK_ARG(ldg >= C && ldg % 4 == 0 && ldx >= C && ldx % 4 == 0 && ldo >= C, "%s: row strides must be >= C (g, x: multiples of 4)", who);
  FF_CHECK_ARG((((uintptr_t)g) & 15) == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)w_frags) & 15) == 0 && (!B || (((uintptr_t)sca) & 15) == 0),
               "%s: 16-byte alignment required", who);
  FF_CHECK_ARG(out != g && out != x, "%s: out must not alias g or x", who);
  NafTailParams p{};
  p.g = g; p.x = x; p.out = out; p.w = (const __bf16*)w_frags; p.sca = sca; p.b3 = b3; p.beta = beta; p.gamma_ln = gamma_ln;
  p.beta_ln = beta_ln; p.b4 = b4; p.b5 = b5; p.oscale = out_scale; p.M = M; p.ldg = ldg; p.ldx = ldx; p.ldo = ldo; p.eps = eps;
  p.rpi = rows_per_image; p.nimg = B ? B : 1;
  hipStream_t st = (hipStream_t)stream;
  if (!B) return C == 64 ? launch_naf_tail<4, 4, 2>(p, st) : launch_naf_tail<8, 4, 1>(p, st);
  return C == 64 ? launch_naf_tail<4, 4, 2, true>(p, st) : launch_naf_tail<8, 4, 1, true>(p, st);
}

extern "C" int ff_naf_tail(const float* g, int ldg, const float* x, int ldx, float* out, int ldo, long long M, int C,
                           const float* sca, const float* b3, const float* beta, const float* gamma_ln, const float* beta_ln,
                           float eps, const void* w_frags, const float* b4, const float* b5, const float* out_scale, void* stream) {
  return naf_tail_launch("ff_naf_tail", g, ldg, x, ldx, out, ldo, M, C, sca, 0, 0, b3, beta, gamma_ln, beta_ln, eps, w_frags, b4, b5, out_scale, stream);
}

// B independent images' rows in one launch: sca [B][C], rows b * rows_per_image .. of g / x / out are image b's.  Every row comes out
// with the bits of ff_naf_tail on its image alone (a row's arithmetic does not depend on the tile or the workgroup that holds it).
// rows_per_image must be a multiple of 32 -- a wave's 32 rows then belong to one image -- and M == B * rows_per_image < 2^31.
extern "C" int ff_naf_tail_images(const float* g, int ldg, const float* x, int ldx, float* out, int ldo, long long M, int C,
                                  const float* sca, int B, int rows_per_image, const float* b3, const float* beta, const float* gamma_ln,
                                  const float* beta_ln, float eps, const void* w_frags, const float* b4, const float* b5,
                                  const float* out_scale, void* stream) {
  FF_CHECK_ARG(B >= 1 && rows_per_image > 0 && rows_per_image % 32 == 0,
               "ff_naf_tail_images: rows_per_image must be a positive multiple of 32 (got B=%d rows_per_image=%d)", B, rows_per_image);
  FF_CHECK_ARG(M == (long long)B * rows_per_image && M < (1LL << 31), "ff_naf_tail_images: M must be B * rows_per_image and below 2^31 (got M=%lld)", M);
  return naf_tail_launch("ff_naf_tail_images", g, ldg, x, ldx, out, ldo, M, C, sca, B, rows_per_image, b3, beta, gamma_ln, beta_ln, eps, w_frags, b4, b5, out_scale, stream);
}
