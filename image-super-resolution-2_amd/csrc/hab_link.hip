// HAB link (plain bf16): block i's tail and block i+1's head in ONE launch,
//     x_out = x1 + fc2(GELU(fc1(LayerNorm2(x1)))),  x1 = x + proj(att_i) + c2 * gate          (token_projmlp_bf16_kernel, block i)
//     xn = LayerNorm1(x_out),  att_{i+1} = (S)W-MSA(xn)                                        (win_attn_fused_v2_kernel<16, true>, block i+1)
// The stand-alone pair writes x_out (47 MB of fp32 at 65 536 tokens) and the attention's first act is to gather the same rows back
// (17.7 us of its 62.5 with nothing under it).  token_projmlp is per token, so it may be tiled by ANY partition of the tokens: here a
// workgroup is one (shifted) 16 x 16 window of block i+1 and wave w, accumulator row r is window position 32 w + r.  A wave then
// finishes phase A holding the final x of exactly the 32 positions it normalises in phase B, and hands them over through its own LDS
// patch -- no workgroup barrier, no HBM read.  x_out is still stored (it is block i+1's residual).
//
// The arithmetic is the parents', statement for statement, because every phase they share is the SAME TEXT:
//   phase A   token_projmlp_bf16_dma.inc (projection image, W1 / W2 slot maps), token_projmlp_bf16_proj.inc (projection MFMAs),
//             token_projmlp_bf16_ln.inc (norm2 from the accumulators; statistics: token_projmlp_ln_stats.inc), token_projmlp_bf16_mlp.inc
//             (hidden-tile loop) -- they name a field of TokenProjMlpParams PM_P(f), here p.a_f;
//   phase B   win_attn_fused_v2_dma.inc (per-head weight image and bias table), win_attn_fused_v2_ln.inc (norm1), win_attn_fused_v2_heads.inc
//             (per-head loop).
// What stays inline differs on purpose: the att fragments and residual slices (tok_of, bf16 rows only) and the hand-over.  The value
// handed over is what the stand-alone epilogue stores (accumulator + b2 in fp32, zero in the padded channels as the gather leaves
// them).  Results are bit equal to ff_token_projmlp_images followed by ff_win_attn_fused.
//
// LDS (one image, both phases; offsets of token_mlp_layout.h and win_attn_layout.h):
//   phase A   [0, 78 K) projection image, then the W1 / W2 double buffers | [78 K, 146 K) wave patches (residual transposes) | vectors
//   phase B   [0, 38 K) a head's weight image | [38 K, 78 K) K x 2 | [78 K, 111 K) V^T x 2 | bias tables x 2 | projection biases
//   both      above phase A's vectors: gamma1 | beta1 | b2 | the image's gate row | block i's projection bias, copied once in the prologue
//             (a global read of them later would queue behind the bulk traffic that is in flight by then)
// Order at the boundary: the hidden-tile loop ends with a workgroup barrier (every wave is past the W1 / W2 slots and, long before,
// the phase-A patches), so head 0's weight image, its bias table and the projection biases are fetched right there, onto areas no
// wave touches again in phase A.  The hand-over patch is where the stand-alone attention keeps its gather patch (over the K / V area,
// clear of all three), and the per-head loop's first barrier orders every wave's last patch read before the first K / V^T write.
#include "ff_common.h"
#include "win_geometry.h"
#include "token_mlp_layout.h"
#include "win_attn_layout.h"

#define HL_OFF_VEC PM_OFF_VEC                            // gamma2 | beta2 | b1: above every phase-B area, so phase B may be prefetched under phase A's tail
#define HL_K 180
#define HL_HEADS 6

struct HabLinkParams {
  // ---- block i (the names of TokenProjMlpParams, a_ prefixed)
  const __bf16* a_att; const float* a_x; const __bf16* a_c2; const float* a_rs2; float* a_out;
  const float* a_gamma; const float* a_beta; const __bf16* a_wp; const float* a_bp; const __bf16* a_w; const float* a_b1; const float* a_b2;
  int a_lda, a_ldx, a_ldc, a_ldo, a_rs2_ld, HT;
  float a_eps;
  // ---- block i+1 (the names of WinFusedParams, which the shared text reads; what the entry point fixes is a constant here)
  float* out; const float* gamma; const float* beta; const __bf16* w; const float* bias; const float* rel; float* xn;
  int ldo, ldxn, o_off, H, W, sh, sw, use_mask, nwx, nwy, rel_rows, rel_stride;
  int K;                  // 180, but a run-time value as in the parents: their LayerNorm statements must compile to the same mix of fused and unfused
                          // multiply-adds (with a constant K the compiler drops the padded channels' terms and contracts different ones)
  float eps;
  static constexpr int d = 30, head0 = 0, nheads = HL_HEADS, out_bf16 = 1, xn_bf16 = 1, ldv = 0, v_off = 0;
  static constexpr float* vout = nullptr;
  FF_STAMP_MEMBER
};

#define HL_OFF_VEC_B (HL_OFF_VEC + (2 * TM_KP + 12 * 32) * 4)     // gamma1 | beta1 | b2 | gate row | projection bias: read once, in the prologue
#define HL_LDS (HL_OFF_VEC_B + 5 * TM_KP * 4)
static_assert(HL_LDS <= FF_LDS_MAX, "LDS image too large");
static_assert(W2_LDS <= PM_OFF_VEC, "the attention's tables must stay below phase A's vectors");
static_assert(W2_WB <= PM_PROJB && W2_OFF_K + 8 * 32 * WF_XS_ROW * 4 <= W2_OFF_REL, "hand-over patches must clear the weight image and the bias tables");
#define PM_P(f) p.a_##f                                // the shared phase-A texts' name for field f of TokenProjMlpParams

__global__ __launch_bounds__(512) void hab_link_kernel(HabLinkParams p) {
  constexpr int WW = 16, WH = 16, RS = 48, TPR = 2, WWM = 16;
  constexpr bool ONES = true;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Gs = reinterpret_cast<float*>(smem + HL_OFF_VEC);
  float* Bts = Gs + TM_KP;
  float* B1s = Bts + TM_KP;
  float* G1s = reinterpret_cast<float*>(smem + HL_OFF_VEC_B);           // LayerNorm1's gamma / beta, the hand-over's b2, the image's gate row
  float* Bt1s = G1s + TM_KP;
  float* B2s = Bt1s + TM_KP;
  float* Scs = B2s + TM_KP;
  float* Bps = Scs + TM_KP;                                             // the padded projection bias (token_projmlp_bf16_proj.inc)
  float* Bs = reinterpret_cast<float*>(smem + W2_OFF_BS);
  unsigned* same = reinterpret_cast<unsigned*>(smem + W2_OFF_SAME);     // (the ONES form never reads it)
  const int* ktok = nullptr;                                            // (only the v side output reads it: absent here)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const FFWinId win = ff_win_decode(blockIdx.x, p.nwx, p.nwy);
  const int wx = win.wx, wy = win.wy, b = win.b;            // image: its gate row, its tokens
  float* patch = reinterpret_cast<float*>(smem + PM_OFF_PATCH + wid * PM_PATCHB);
  // window position -> token (the cyclic shift is index arithmetic; H and W are multiples of 16, so every position is a token)
  auto tok_of = [&](int pos) {
    FF_WIN_UNSHIFT_DECL(oy, ox, wy * WH + (pos >> 4), wx * WW + (pos & 15), p.sh, p.sw, p.H, p.W);      // (the text form: a call moves registers)
    return (b * p.H + oy) * p.W + ox;
  };
  FF_STAMP(128, 0);

  // ================================================ phase A: block i's projection + residuals + norm2 + MLP ======================
#include "token_projmlp_bf16_dma.inc"
  for (int i = tid; i < p.HT * 32; i += 512) B1s[i] = p.a_b1[i];
  if (tid < TM_KP) { Gs[tid] = tid < p.K ? p.a_gamma[tid] : 0.f; Bts[tid] = tid < p.K ? p.a_beta[tid] : 0.f; }
  // phase B's vectors and the gate row, read once here: by the time they are needed every workgroup has its x_out stores in flight, and
  // a global read would queue behind them.  The padded channels hold zero; the selects that keep them out of a result stay as they are.
  if (tid >= 256 && tid < 256 + TM_KP) {
    const int c = tid - 256;
    const bool cok = c < p.K;
    G1s[c] = cok ? p.gamma[c] : 0.f; Bt1s[c] = cok ? p.beta[c] : 0.f; B2s[c] = cok ? p.a_b2[c] : 0.f;
    Scs[c] = cok ? p.a_rs2[(long long)b * p.a_rs2_ld + c] : 0.f;
    Bps[c] = p.a_bp[c];
  }

  // ---- att rows (bf16) -> fragments: a lane's fragment of k-step st IS 16 bytes of its token's row ---------------------------
  bf16x8 xh[TM_KS];
  {
    const __bf16* arow = p.a_att + tok_of(wid * 32 + l31) * p.a_lda + 8 * hh;
#pragma unroll
    for (int st = 0; st < TM_KS; ++st) xh[st] = *reinterpret_cast<const bf16x8*>(arow + 16 * st);      // all twelve in flight, then the masks
#pragma unroll
    for (int st = 0; st < TM_KS; ++st) {
      if (16 * st + 8 * hh + 7 >= p.K) {               // the row's padding is never written: mask it
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (16 * st + 8 * hh + j >= p.K) xh[st][j] = (__bf16)0.f;
      }
    }
  }
  FF_STAMP(128, 1);

  // ---- residual slices: coalesced float4 loads (lane = window position lane>>3 (+8i) of the wave, channel quad), one slice ahead:
  //      two register sets, slice n + 1 is issued before slice n is consumed; slices 0 and 1 go out right behind the barrier below
  //      and land under the projection's MFMAs (issued before the wait in front of that barrier, slice 0 only lengthened the wait:
  //      profiles/hab_link_prefetch.json).  c2 stays the bf16 it is loaded as until it is consumed (the conversion is exact), so that
  //      nothing waits for a slice before its turn.
  const int tq = lane >> 3, q4 = 4 * (lane & 7);
  f32x4 rx[2][4];
  bf16x4 rc[2][4];
  // 32-bit element offsets of the lane's four token rows (entry point: B H W ld < 2^31); channels past K read channel 0 instead --
  // finite values that the zero-padded gamma / beta keep out of fc1 and that the hand-over replaces by zero
  int xo[4], co[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = tok_of(wid * 32 + tq + 8 * i);
    xo[i] = t * p.a_ldx + q4;
    co[i] = t * p.a_ldc + q4;
  }
  auto load_res = [&](int n) {
    const int cn = (n * 32 + q4 < p.K) ? n * 32 : -q4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rx[n & 1][i] = *reinterpret_cast<const f32x4*>(p.a_x + (xo[i] + cn));
      rc[n & 1][i] = *reinterpret_cast<const bf16x4*>(p.a_c2 + (co[i] + cn));
    }
  };
  // vmcnt(0) lgkmcnt(0), as the builtin and not as text: the compiler then knows that nothing is in flight behind it.  After an LDS-DMA
  // it otherwise makes the next use of a loaded register wait for EVERY load issued before that use -- the slices below included
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0x0070);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();                          // the projection image, the vectors and the fragments are in place
  load_res(0);                                           // 16.7 MB a slice over all workgroups: they land under the projection's MFMAs
  load_res(1);

#include "token_projmlp_bf16_proj.inc"
  FF_STAMP(128, 2);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                          // every wave is past the projection image: the MLP's first two tiles may land on it
  FF_STAMP(128, 3);
  dma_mlp(0, 0);
  if (p.HT > 1) dma_mlp(1, 1);
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    // x1 = proj + shortcut + conv * scale, slice n: through the wave's patch into accumulator order
    if (n >= 1 && n + 1 < 6) load_res(n + 1);            // (slices 0 and 1 left before the projection)
    const int c4 = n * 32 + q4;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(Scs + c4);        // the image's gate, zero in the padded channels
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 r0 = rx[n & 1][i];
      const bf16x4 h4 = rc[n & 1][i];
      r0 += (f32x4){(float)h4[0], (float)h4[1], (float)h4[2], (float)h4[3]} * sc;
      *reinterpret_cast<f32x4*>(patch + (tq + 8 * i) * 36 + q4) = r0;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 u = *reinterpret_cast<const f32x4*>(patch + l31 * 36 + 8 * g + 4 * hh);
#pragma unroll
      for (int e = 0; e < 4; ++e) oacc[n][4 * g + e] += u[e];
    }
  }
  FF_STAMP(128, 4);

  // ---- LayerNorm(x1) from the accumulators -> fc1 operand --------------------------------------------------------------------
#include "token_projmlp_bf16_ln.inc"
  FF_STAMP(128, 5);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                          // tiles 0 and 1 of the MLP have landed
  FF_STAMP(128, 6);

#define PM_STAMP(i) FF_STAMP(128, i)
#include "token_projmlp_bf16_mlp.inc"
#undef PM_STAMP
  FF_STAMP(128, 40);

  // ================================================ the boundary =================================================================
  // The loop above ended with a workgroup barrier: the W1 / W2 slots and phase A's patches are idle in every wave.  Head 0's weight
  // image (38 one-KiB pieces, 5 per wave), its bias table and the q / k / v biases go out now and land under the hand-over.
#include "win_attn_fused_v2_dma.inc"
  dma_head(0, 0);
  // q / k / v biases; padded V channel 30 is the constant 1 (the denominator channel).  Visible after the head loop's first barrier.
  for (int i = tid; i < 3 * HL_HEADS * 32; i += 512) Bs[i] = (i % 96 == 94) ? 1.0f : p.bias[i];

  const bool blk_mask = p.use_mask && ff_win_has_regions(wx, wy, p.nwx, p.nwy);
  const int qi = wid * 32 + 31 - l31;                  // this lane's window position in phase B (query; also one of the wave's keys)
  const int mytok = tok_of(qi);
  constexpr bool tvalid = true, kill_pad = false;
  constexpr unsigned vmask = 0xffffffffu;
  const int qreg_id = p.use_mask ? ff_win_region(wy * WH + qi / WW, wx * WW + qi % WW, p.H, p.W, WH, WW, p.sh, p.sw) : 0;
  const float msy = (qreg_id / 3 == 2) ? -7.0625f : 7.0625f, msx = (qreg_id % 3 == 2) ? -7.0625f : 7.0625f;

  // ---- hand-over: x_out = accumulators + b2 leaves through the wave's patch twice -- as 128-byte row segments to memory (block
  //      i+1's residual) and as the attention's fragment rows (lane l31 = window position 32 w + 31 - l31), 64 channels per pass.
  //      Padded channels are handed over as zero: that is what the stand-alone gather leaves there, and the LayerNorm sum runs
  //      over them.
  {
    float* xs = reinterpret_cast<float*>(smem + W2_OFF_K) + wid * (32 * WF_XS_ROW);
    float v[WF_KS][8];
    int oo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) oo[i] = tok_of(wid * 32 + tq + 8 * i) * p.a_ldo + q4;
    const float* xrow = xs + (31 - l31) * WF_XS_ROW + 8 * hh;
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int n = 2 * pass + h2;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int c0 = n * 32 + 8 * g + 4 * hh;
          const bool cok = c0 < p.K;
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(B2s + (cok ? c0 : 0));
          f32x4 v4;
#pragma unroll
          for (int e = 0; e < 4; ++e) v4[e] = cok ? oacc[n][4 * g + e] + b4[e] : 0.f;
          *reinterpret_cast<f32x4*>(xs + l31 * WF_XS_ROW + 32 * h2 + 8 * g + 4 * hh) = v4;
        }
      }
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int cn = (2 * pass + h2) * 32;
        f32x4 ov[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) ov[i] = *reinterpret_cast<const f32x4*>(xs + (tq + 8 * i) * WF_XS_ROW + 32 * h2 + q4);
        if (cn + q4 < p.K) {
#pragma unroll
          for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(p.a_out + (oo[i] + cn)) = ov[i];
        }
      }
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(xrow + 16 * s4);
        const f32x4 c4 = *reinterpret_cast<const f32x4*>(xrow + 16 * s4 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[4 * pass + s4][e] = a[e]; v[4 * pass + s4][4 + e] = c4[e]; }
      }
    }
    FF_STAMP(128, 41);
    // this wave's pieces of head 0 have landed (and with them the x_out stores issued above)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FF_STAMP(128, 42);
#define W2_LN(f) ln1_##f                               // LayerNorm1's gamma / beta come from LDS here
    const float* const ln1_gamma = G1s;
    const float* const ln1_beta = Bt1s;
#include "win_attn_fused_v2_ln.inc"
#undef W2_LN
  }
  FF_STAMP(128, 64 + 2);

  // ================================================ phase B: block i+1's heads ======================================================
#define W2_STAMP(i) FF_STAMP(128, 64 + (i))
#include "win_attn_fused_v2_heads.inc"
#undef W2_STAMP
  FF_STAMP(128, 64 + 60);
  FF_STAMP_DRAINED(128, 64 + 61);
}
#undef PM_P

extern "C" int ff_hab_link(const float* att, int lda, const float* x, int ldx, const float* c2, int ldc, const float* c2_scale,
                           int scale_ld, int B, long long rows_per_image, float* x_out, int ldxo, long long M, int K, int hidden_tiles,
                           const void* proj_tiles, const float* proj_bias_padded, const float* gamma2, const float* beta2, float eps2,
                           const void* mlp_tiles, const float* b1_padded, const float* b2, int nterms, int io_bf16,
                           float* att_out, int ldo, int o_off, const float* gamma1, const float* beta1, float eps1,
                           const void* qkv_tiles, const float* qkv_bias_padded, const float* rel_padded, int rel_rows, int rel_stride,
                           int H, int W, int wh, int ww, int shift_h, int shift_w, int use_mask, int nheads, int d,
                           float* xn_out, int ldxn, int out_bf16, int xn_bf16, void* stream) {
  // ---- what the kernel is not built for is refused here, before anything is launched
  FF_CHECK_ARG(nterms == 1, "ff_hab_link: plain bf16 only (nterms must be 1)");
  FF_CHECK_ARG(wh == 16 && ww == 16, "ff_hab_link: the window must be 16x16 (got %dx%d)", wh, ww);
  FF_CHECK_ARG(d == 30 && nheads == HL_HEADS, "ff_hab_link: six heads of dim 30 only (got %d x %d)", nheads, d);
  FF_CHECK_ARG(K == HL_K, "ff_hab_link: K must be 180 (got %d)", K);
  FF_CHECK_ARG(B > 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "ff_hab_link: H and W must be positive multiples of 16 (got %dx%d)", H, W);
  FF_CHECK_ARG(io_bf16 == 3 && out_bf16 == 1 && xn_bf16 == 1, "ff_hab_link: att, c2, xn_out and att_out are bf16 rows (fp32 rows are refused)");
  FF_CHECK_ARG(c2 && c2_scale, "ff_hab_link: c2 and the gate are required");
  FF_CHECK_ARG(att && x && x_out && proj_tiles && proj_bias_padded && gamma2 && beta2 && mlp_tiles && b1_padded && b2 && att_out && gamma1 && beta1 &&
               qkv_tiles && qkv_bias_padded && rel_padded && xn_out, "ff_hab_link: null pointer");
  FF_CHECK_ARG(rows_per_image == (long long)H * W && M == (long long)B * rows_per_image, "ff_hab_link: rows_per_image must be H * W and M must be B * rows_per_image");
  FF_CHECK_ARG(hidden_tiles > 0 && hidden_tiles <= 12, "ff_hab_link: at most 12 hidden tiles (got %d)", hidden_tiles);
  FF_CHECK_ARG(lda % 8 == 0 && lda >= 192 && ldc % 4 == 0 && ldc >= K && (((uintptr_t)att) & 15) == 0 && (((uintptr_t)c2) & 7) == 0,
               "ff_hab_link: bf16 att rows must be 16-byte aligned and padded to 192 channels, c2 rows 8-byte aligned");
  FF_CHECK_ARG(ldx % 4 == 0 && ldx >= K && ldxo % 4 == 0 && ldxo >= K && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)x_out) & 15) == 0,
               "ff_hab_link: x / x_out rows must be 16-byte aligned");
  FF_CHECK_ARG(scale_ld >= K && scale_ld % 4 == 0 && (((uintptr_t)c2_scale) & 15) == 0, "ff_hab_link: gate rows must be 16-byte aligned (scale_ld >= K, scale_ld %% 4 == 0)");
  FF_CHECK_ARG(ldxn % 8 == 0 && ldxn >= 192 && (((uintptr_t)xn_out) & 15) == 0, "ff_hab_link: bf16 xn rows must be 16-byte aligned and padded to 192 channels");
  FF_CHECK_ARG(ldo % 2 == 0 && o_off % 2 == 0 && o_off >= 0 && (((uintptr_t)att_out) & 7) == 0 && ldo >= o_off + nheads * d, "ff_hab_link: att_out rows must be 8-byte aligned and hold every head");
  FF_CHECK_ARG((((uintptr_t)proj_tiles) & 15) == 0 && (((uintptr_t)mlp_tiles) & 15) == 0 && (((uintptr_t)qkv_tiles) & 15) == 0 && (((uintptr_t)rel_padded) & 15) == 0 &&
               (((uintptr_t)gamma1) & 15) == 0 && (((uintptr_t)beta1) & 15) == 0 && (((uintptr_t)b2) & 15) == 0,
               "ff_hab_link: weights / bias table / gamma1 / beta1 / b2 must be 16-byte aligned");
  FF_CHECK_ARG(shift_h >= 0 && shift_w >= 0 && shift_h < wh && shift_w < ww, "ff_hab_link: bad shift");
  FF_CHECK_ARG(!use_mask || (shift_h > 0 && shift_w > 0), "ff_hab_link: mask needs a shift");
  FF_CHECK_ARG(rel_rows == 2 * wh - 1 && rel_stride == 48, "ff_hab_link: bias table must be [heads][31][stride 48]");
  {
    int ldmax = lda > ldx ? lda : ldx;
    if (ldc > ldmax) ldmax = ldc;
    if (ldxo > ldmax) ldmax = ldxo;
    if (ldo > ldmax) ldmax = ldo;
    if (ldxn > ldmax) ldmax = ldxn;
    FF_CHECK_ARG(M * (long long)ldmax < (1LL << 31), "ff_hab_link: too many tokens for 32-bit row offsets (B * H * W * ld must be < 2^31)");
  }
  HabLinkParams p;
  p.a_att = (const __bf16*)att; p.a_x = x; p.a_c2 = (const __bf16*)c2; p.a_rs2 = c2_scale; p.a_out = x_out;
  p.a_gamma = gamma2; p.a_beta = beta2; p.a_wp = (const __bf16*)proj_tiles; p.a_bp = proj_bias_padded; p.a_w = (const __bf16*)mlp_tiles;
  p.a_b1 = b1_padded; p.a_b2 = b2; p.a_lda = lda; p.a_ldx = ldx; p.a_ldc = ldc; p.a_ldo = ldxo; p.a_rs2_ld = scale_ld; p.HT = hidden_tiles;
  p.a_eps = eps2;
  p.out = att_out; p.gamma = gamma1; p.beta = beta1; p.w = (const __bf16*)qkv_tiles; p.bias = qkv_bias_padded; p.rel = rel_padded; p.xn = xn_out;
  p.ldo = ldo; p.ldxn = ldxn; p.o_off = o_off; p.H = H; p.W = W; p.sh = shift_h; p.sw = shift_w; p.use_mask = use_mask;
  p.nwx = W / ww; p.nwy = H / wh; p.rel_rows = rel_rows; p.rel_stride = rel_stride; p.eps = eps1; p.K = K;
  FF_STAMP_ARM(p);
  const long long nblk = (long long)B * p.nwx * p.nwy;
  FF_CHECK_ARG(nblk < (1LL << 31), "ff_hab_link: grid too large");
  static ff_device_once once;
  if (!ff_raise_lds(once, "ff_hab_link", HL_LDS, FF_LDS_SAY_ERR, &hab_link_kernel)) return FF_ERR_LAUNCH;
  hipLaunchKernelGGL(hab_link_kernel, dim3((unsigned)nblk), dim3(512), HL_LDS, (hipStream_t)stream, p);
  FF_LAUNCH_CHECK("ff_hab_link");
  return FF_OK;
}
