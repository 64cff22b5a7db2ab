// Fused transformer MLP on tokens:  out = x + fc2( GELU( fc1( LayerNorm(x) ) ) )      (hat_arch.py:83-94,307;
// the HAB / OCAB feed-forward, 84 per HAT forward).  One launch instead of LayerNorm + 2 GEMMs, and the
// hidden activation (360 floats per token) never leaves the CU: HBM traffic is x in, out out (94 MB per call at
// 65 536 tokens instead of 423 MB), which is what bounds these K=180 layers.
//
// "Flash-MLP" dataflow, split-operand bf16 MFMA (v_mfma_f32_32x32x16_bf16, fp32 accumulate, bf16x3):
//   * a wave owns 32 tokens; LayerNorm(x) of those tokens is the B operand of every k-step (lane = token, 8 consecutive
//     k per lane and step), produced once: the hi halves live in REGISTERS (48 VGPRs), the lo halves in a wave-private
//     LDS image (keeping both in registers next to the 96 output accumulators overflows the 256-VGPR budget);
//   * per 32-wide hidden tile:  H^T[hidden][token] = W1 . LN(x)^T  (A = W1 rows from LDS), bias, GELU, split to bf16;
//     the accumulator has hidden on the registers and the token on the lane, so it IS the B operand of
//     OUT^T[n][token] += W2[n][hidden] . H^T   (guide section 3, 'An accumulator tile as the next MFMA's operand';
//     W2's hidden columns are stored in the matching permuted order: bits 2 and 3 of the index swapped);
//   * weight tiles (W1: 32 x 192, W2: 192 x 32, hi + lo planes) are shared by the 8 waves of the workgroup and filled by
//     LDS-DMA (global_load_lds_dwordx4: no VGPRs, no staging stores).  The LDS images are 25 + 30 lane-linear 1-KiB
//     pieces; rows are padded by one 16-byte slot (conflict-free ds_read_b128) and the per-lane SOURCE address does the
//     row/pad bookkeeping (guide section 5, Caveat).  Two barriers per hidden tile: W1 is refilled for tile t+1 while
//     GELU + GEMM2 of tile t run, W2 while GEMM1 of tile t+1 runs;
//   * epilogue: 32x32 tiles are transposed through LDS so global stores / residual loads are 128-byte row segments.
// Workgroup = 8 waves = 256 tokens: 65 536 tokens -> 256 workgroups = one per CU.
#include "ff_common.h"

#include "token_mlp_layout.h"

struct TokenMlpParams {
  const float* x; float* out;
  const float* gamma; const float* beta;
  const __bf16* w;        // [HT][4 planes: W1hi, W1lo, W2hi, W2lo][6144]; W2 planes are [192][32] with permuted hidden columns
  const float* b1;        // [HT*32] zero padded
  const float* b2;        // [N]
  long long M;
  int ldx, ldo, K, N, HT;
  float eps;
};

template <bool VEC4, int NTERMS>
__global__ __launch_bounds__(512) void token_mlp_kernel(TokenMlpParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int W1B = TM_W1B, W2B = TM_W2B;          // the map: token_mlp_layout.h
  unsigned char* W1s = smem;                         // [2 planes][32][400]
  unsigned char* W2s = smem + TM_OFF_W2;             // [2 planes][192][80]
  unsigned char* XLs = smem + TM_OFF_XL;             // [8 waves][32 tokens][400]
  float* B1s = reinterpret_cast<float*>(smem + TM_OFF_B1);   // [HT*32] fc1 bias (read every hidden tile)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const long long tok = (long long)blockIdx.x * 256 + wid * 32 + l31;
  const bool tvalid = tok < p.M;

#include "token_mlp_split_dma.inc"
  dma_w1(0);
  dma_w2(0);
  for (int i = tid; i < p.HT * 32; i += 512) B1s[i] = p.b1[i];

  // ---- LayerNorm(x) of this lane's token half -> bf16 hi (registers) / lo (wave-private LDS rows) -----------------
  bf16x8 xh[TM_KS];
  unsigned char* xl_row = XLs + (size_t)(wid * 32 + l31) * XLROWB + 16 * hh;     // + 32*st per k-step
  {
    float v[TM_KS][8];
    // staging patch = this wave's own x_lo rows (12.8 KB, written only below, after the fragments are in registers)
    ff_wave_rows_to_frags<3>(p.x, p.ldx, (long long)blockIdx.x * 256 + wid * 32, p.M, p.K,
                          reinterpret_cast<float*>(XLs + (size_t)wid * 32 * XLROWB), lane, v);
    float mean, rstd;
    ff_frag_ln_stats<TM_KS>(v, p.K, hh, p.eps, mean, rstd);
#pragma unroll
    for (int st = 0; st < TM_KS; ++st) {
      float f[8];
      ff_frag_ln_step(v[st], p.gamma, p.beta, 16 * st + 8 * hh, p.K, mean, rstd, f);
      bf16x8 lo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        __bf16 h, l;
        ff_bf16_split(f[j], h, l);
        xh[st][j] = h;
        lo[j] = l;
      }
      *reinterpret_cast<bf16x8*>(xl_row + 32 * st) = lo;
    }
  }

  f32x16 oacc[6];
#pragma unroll
  for (int n = 0; n < 6; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[n][r] = 0.f;

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // tile 0 landed (this wave's pieces)
  __syncthreads();

#define TM_NTERMS NTERMS
#define TM_STAMP(i) do { } while (0)                   // (TokenMlpParams has no stamp member)
#include "token_mlp_split_tiles.inc"
#undef TM_STAMP
#undef TM_NTERMS

  // ---- epilogue: all 96 residual loads first (x fragments are dead, registers are free), then per n-tile a
  // transpose through LDS -> coalesced 128-byte row segments.  (out may alias x as far as the compiler knows: a
  // load placed after a store would be serialised behind it.)
  const long long tok0 = (long long)blockIdx.x * 256 + wid * 32;
  if (VEC4) {
    // 16-byte form: the accumulator's four consecutive channels per r >> 2 go to the patch as one ds_write_b128, a lane
    // then owns (token row lane >> 3 (+8 per step), channel quad lane & 7): one float4 residual load and one float4
    // store per step = 8 whole 128-byte row segments per instruction (2 with dword accesses)
    float* tr = reinterpret_cast<float*>(smem) + wid * (32 * 36);    // per-wave [token][36] over the (now idle) W images
    static_assert(TM_TRB(36) <= TM_OFF_XL, "the transpose patches must stay inside the W images");
    const int tq = lane >> 3, q4 = 4 * (lane & 7);
    f32x4 rq[6][4];
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      const int c4 = n * 32 + q4;
      const bool cok = c4 < p.N;
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.b2 + (cok ? c4 : 0));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long tk = tok0 + tq + 8 * i;
        const f32x4 u = *reinterpret_cast<const f32x4*>(p.x + (tk < p.M ? tk : 0) * p.ldx + (cok ? c4 : 0));
        rq[n][i] = u + b4;
      }
    }
#pragma unroll
    for (int n = 0; n < 6; ++n) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v4;
#pragma unroll
        for (int e = 0; e < 4; ++e) v4[e] = oacc[n][4 * g + e];
        *reinterpret_cast<f32x4*>(tr + l31 * 36 + 8 * g + 4 * hh) = v4;
      }
      f32x4 ov[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ov[i] = *reinterpret_cast<const f32x4*>(tr + (tq + 8 * i) * 36 + q4) + rq[n][i];
      const int c4 = n * 32 + q4;
      if (c4 < p.N) {
        float* op = p.out + (tok0 + tq) * p.ldo + c4;
        if (tok0 + 32 <= p.M) {
#pragma unroll
          for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(op + (long long)(8 * i) * p.ldo) = ov[i];
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (tok0 + tq + 8 * i < p.M) *reinterpret_cast<f32x4*>(op + (long long)(8 * i) * p.ldo) = ov[i];
        }
      }
    }
    return;
  }
  float* tr = reinterpret_cast<float*>(smem) + wid * (32 * 33);    // per-wave [token][33] over the (now idle) W images
  static_assert(TM_TRB(33) <= TM_OFF_XL, "the transpose patches must stay inside the W images");
  float rv[6][16];
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    const int col = n * 32 + l31;
    const int cc = col < p.N ? col : 0;
    const float bias = col < p.N ? p.b2[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long long tk = tok0 + 2 * i + hh;
      rv[n][i] = p.x[(tk < p.M ? tk : 0) * p.ldx + cc] + bias;
    }
  }
#pragma unroll
  for (int n = 0; n < 6; ++n) {
#pragma unroll
    for (int r = 0; r < 16; ++r) tr[l31 * 33 + (r & 3) + 8 * (r >> 2) + 4 * hh] = oacc[n][r];
    const int col = n * 32 + l31;
    float ov[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) ov[i] = tr[(2 * i + hh) * 33 + l31] + rv[n][i];
    if (col < p.N) {
      float* op = p.out + (tok0 + hh) * p.ldo + col;
      if (tok0 + 32 <= p.M) {
#pragma unroll
        for (int i = 0; i < 16; ++i) op[(long long)(2 * i) * p.ldo] = ov[i];
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (tok0 + 2 * i + hh < p.M) op[(long long)(2 * i) * p.ldo] = ov[i];
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// Attention output projection + residuals + norm2 + MLP in ONE launch (HAB / OCAB tail, hat_arch.py:303-307):
//     x1  = shortcut + proj(att) + conv_x * conv_scale            (:305; the conv term is absent in OCAB :436)
//     out = x1 + fc2(GELU(fc1(LayerNorm(x1))))                    (:307 / :437)
// The two-kernel form (token_linear proj -> token_mlp) wrote x1 (47 MB) and read it back; here the six 32-channel tiles of
// proj^T[channel][token] stay in the 96 output accumulators: the residuals are added there, the LayerNorm statistics are taken
// from them (a lane holds 96 of its token's 192 padded channels, the other half sits in lane + 32), the normalised values
// become the fc1 operand straight from the accumulator registers -- registers 8s..8s+7 of tile n are k-step 2n+s, so fc1's
// K columns are stored in the matching permuted order (prep.pack_token_projmlp) -- and x1 itself remains in the
// accumulators as the final residual.  att rows are the B operand of the projection (hi in registers, lo in the wave's
// LDS rows, like x in token_mlp); the projection's weight tiles use the W1 / W2 image areas as a 2-slot ring.
struct TokenProjMlpParams {
  const float* att; const float* x; const float* c2; const float* rs2;   // c2 / rs2 may be NULL (OCAB)
  float* out;
  const float* gamma; const float* beta;
  const __bf16* wp;       // proj tiles [6][2 planes][32][192]
  const float* bp;        // [192] proj bias, zero padded
  const __bf16* w;        // MLP tiles as in TokenMlpParams, W1 columns permuted
  const float* b1; const float* b2;
  long long M;
  int lda, ldx, ldc, ldo, K, N, HT;
  float eps;
  int io_bf16;            // plain-bf16 kernel only: bit 0 = att rows are bf16 (lda in elements), bit 1 = c2 rows are bf16 (ldc in elements)
  int wpi, rs2_ld;        // per-image gate (ff_token_projmlp_images): image blockIdx.y reads rs2 + blockIdx.y * rs2_ld; the grid is
                          // (wpi workgroups per image, images), so the image index costs no division and no vector register
  FF_STAMP_MEMBER
};
#define PM_P(f) p.f                                    // the shared phase texts' name for field f (hab_link.hip: p.a_##f)

__global__ __launch_bounds__(512) void token_projmlp_kernel(TokenProjMlpParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int W1B = TM_W1B, W2B = TM_W2B;
  unsigned char* W1s = smem;
  unsigned char* W2s = smem + TM_OFF_W2;
  unsigned char* XLs = smem + TM_OFF_XL;
  float* B1s = reinterpret_cast<float*>(smem + TM_OFF_B1);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const long long tok0 = ((long long)blockIdx.y * p.wpi + blockIdx.x) * 256 + wid * 32;   // blockIdx.y = image (0 in the single-gate launch)

#include "token_mlp_split_dma.inc"
  // projection tile n (a W1-format image) into ring slot 0 = the W1 area, 1 = the W2 area (30 720 B >= 25 600 B)
  auto dma_proj = [&](int n, int slot) {
    const __bf16* rec = p.wp + (long long)n * (2 * TILE_ELEMS);
    unsigned char* dst = slot ? W2s : W1s;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (wid + 8 * i < W1PIECES)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rec + off1[i]),
                                         (__attribute__((address_space(3))) void*)(dst + (wid + 8 * i) * 1024), 16, 0, 0);
  };
  FF_STAMP(64, 0);
  dma_proj(0, 0);
  for (int i = tid; i < p.HT * 32; i += 512) B1s[i] = p.b1[i];

  // ---- att rows -> split fragments (hi registers, lo in the wave's LDS rows) ---------------------------------------
  bf16x8 xh[TM_KS];
  unsigned char* xl_row = XLs + (size_t)(wid * 32 + l31) * XLROWB + 16 * hh;
  {
    float v[TM_KS][8];
    ff_wave_rows_to_frags<3>(p.att, p.lda, tok0, p.M, p.K, reinterpret_cast<float*>(XLs + (size_t)wid * 32 * XLROWB), lane, v);
#pragma unroll
    for (int st = 0; st < TM_KS; ++st) {
      bf16x8 lo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = v[st][j];
        const __bf16 h = (__bf16)f;
        xh[st][j] = h;
        lo[j] = (__bf16)(f - (float)h);
      }
      *reinterpret_cast<bf16x8*>(xl_row + 32 * st) = lo;
    }
  }

  FF_STAMP(64, 1);
  // ---- proj^T tiles into the output accumulators -------------------------------------------------------------------
  f32x16 oacc[6];
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                        // tile n landed everywhere; every wave is past tile n-1
    if (n + 1 < 6) dma_proj(n + 1, (n + 1) & 1);
    const float* bpn = p.bp + n * 32 + 4 * hh;
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[n][r] = bpn[(r & 3) + 8 * (r >> 2)];
    const unsigned char* ap = ((n & 1) ? W2s : W1s) + l31 * W1ROWB + 16 * hh;
#define TM_NTERMS 3
#define TM_ACC oacc[n]
#include "token_mlp_split_tile_mfma.inc"
#undef TM_ACC
#undef TM_NTERMS
  }
  FF_STAMP(64, 2);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                          // both image areas are free again: start the MLP's first tiles
  FF_STAMP(64, 3);
  dma_w1(0);
  dma_w2(0);

  // ---- residuals: coalesced float4 loads (lane = token row lane>>3 (+8i), channel quad) go through the wave's own LDS rows
  //      (the att_lo image is dead) and come back in accumulator order: x1 = proj + shortcut + conv * scale ------------
  {
    float* tr = reinterpret_cast<float*>(XLs + (size_t)wid * 32 * XLROWB);    // [32 tokens][36] over the wave's own x_lo rows
    static_assert(32 * 36 * 4 <= 32 * XLROWB, "the wave's patch must fit in its x_lo rows");
    const int tq = lane >> 3, q4 = 4 * (lane & 7);
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      const int c4 = n * 32 + q4;
      const bool cok = c4 < p.N;
      f32x4 sc = {0.f, 0.f, 0.f, 0.f};
      if (p.c2 && cok) sc = *reinterpret_cast<const f32x4*>(p.rs2 + (long long)blockIdx.y * p.rs2_ld + c4);
      f32x4 rq[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long tk = tok0 + tq + 8 * i;
        const bool ok = cok && tk < p.M;
        f32x4 r0 = *reinterpret_cast<const f32x4*>(p.x + (ok ? tk * p.ldx + c4 : 0));
        if (p.c2) r0 += *reinterpret_cast<const f32x4*>(p.c2 + (ok ? tk * p.ldc + c4 : 0)) * sc;
        rq[i] = ok ? r0 : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(tr + (tq + 8 * i) * 36 + q4) = rq[i];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(tr + l31 * 36 + 8 * g + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) oacc[n][4 * g + e] += u[e];
      }
    }
  }
  FF_STAMP(64, 4);
  // ---- LayerNorm(x1) from the accumulators -> fc1 operand (hi registers, lo rows) -------------------------------------
  {
#include "token_projmlp_ln_stats.inc"
#pragma unroll
    for (int n = 0; n < 6; ++n)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 lo;
#pragma unroll
        for (int g2 = 0; g2 < 2; ++g2) {
          const int c0 = n * 32 + 8 * (2 * s2 + g2) + 4 * hh;           // channels of registers 8 s2 + 4 g2 .. + 3
          const bool cok = c0 < p.K;
          const f32x4 g4 = *reinterpret_cast<const f32x4*>(p.gamma + (cok ? c0 : 0));
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.beta + (cok ? c0 : 0));
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float f = cok ? (oacc[n][8 * s2 + 4 * g2 + e] - mean) * rstd * g4[e] + b4[e] : 0.f;
            const __bf16 h = (__bf16)f;
            xh[2 * n + s2][4 * g2 + e] = h;
            lo[4 * g2 + e] = (__bf16)(f - (float)h);
          }
        }
        *reinterpret_cast<bf16x8*>(xl_row + 32 * (2 * n + s2)) = lo;
      }
  }
  FF_STAMP(64, 5);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  FF_STAMP(64, 6);

  // ---- the MLP over hidden tiles (W1 columns are permuted to the operand order above) -----------------------------------
#define TM_NTERMS 3
#define TM_STAMP(i) FF_STAMP(64, i)
#include "token_mlp_split_tiles.inc"
#undef TM_STAMP
#undef TM_NTERMS
  FF_STAMP(64, 40);

  // ---- epilogue: out = accumulators (x1 + fc2 part) + b2, transposed through LDS into 128-byte row segments ------------
  {
    float* tr = reinterpret_cast<float*>(smem) + wid * (32 * 36);    // per-wave [token][36] over the (now idle) W images
    static_assert(TM_TRB(36) <= TM_OFF_XL, "the transpose patches must stay inside the W images");
    const int tq = lane >> 3, q4 = 4 * (lane & 7);
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      const int c4 = n * 32 + q4;
      const bool cok = c4 < p.N;
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.b2 + (cok ? c4 : 0));
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v4;
#pragma unroll
        for (int e = 0; e < 4; ++e) v4[e] = oacc[n][4 * g + e];
        *reinterpret_cast<f32x4*>(tr + l31 * 36 + 8 * g + 4 * hh) = v4;
      }
      f32x4 ov[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ov[i] = *reinterpret_cast<const f32x4*>(tr + (tq + 8 * i) * 36 + q4) + b4;
      if (cok) {
        float* op = p.out + (tok0 + tq) * p.ldo + c4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (tok0 + tq + 8 * i < p.M) *reinterpret_cast<f32x4*>(op + (long long)(8 * i) * p.ldo) = ov[i];
      }
    }
  }
  FF_STAMP(64, 41);
  FF_STAMP_DRAINED(64, 42);
}

// ---- plain-bf16 form of token_projmlp (nterms == 1) ----------------------------------------------------------------------------
// Same dataflow and operand orders as the split kernel above; what changes is the schedule (phase timings of the split form,
// tools/pm_time.cpp, 79.5 us per launch: att 8.1 | proj 6.4 | residuals 18.4 | LayerNorm 6.2 | MLP 29.3 = 12 x 2.44 | stores 6.2):
//   * no lo planes: the six projection tiles are ONE 78-KiB LDS image fetched at kernel start (no per-tile barrier), and the
//     MLP's W1 / W2 tiles are double buffered -- one barrier per hidden tile instead of two, each DMA a full tile ahead;
//   * the residual slice n+1 (x, conv) is in flight while slice n is transposed and tile n+1 is projected;
//   * gamma / beta come from LDS; GELU is x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3) -- |error| <= 4.8e-4, a sixteenth
//     of the bf16 rounding the value receives next -- 5 full-rate + 2 transcendental operations instead of 14 + 2.

__global__ __launch_bounds__(512) void token_projmlp_bf16_kernel(TokenProjMlpParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Gs = reinterpret_cast<float*>(smem + PM_OFF_VEC);
  float* Bts = reinterpret_cast<float*>(smem + PM_OFF_BT);
  float* Scs = reinterpret_cast<float*>(smem + PM_OFF_SC);   // the image's gate row (zero without c2 and in the padded channels)
  float* Bps = reinterpret_cast<float*>(smem + PM_OFF_BP);   // the padded projection bias (token_projmlp_bf16_proj.inc)
  float* B1s = reinterpret_cast<float*>(smem + PM_OFF_B1);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const long long tok0 = ((long long)blockIdx.y * p.wpi + blockIdx.x) * 256 + wid * 32;   // blockIdx.y = image (0 in the single-gate launch)
  float* patch = reinterpret_cast<float*>(smem + PM_OFF_PATCH + wid * PM_PATCHB);      // the wave's gather / transpose patch
  FF_STAMP(64, 0);

#include "token_projmlp_bf16_dma.inc"
  for (int i = tid; i < p.HT * 32; i += 512) B1s[i] = p.b1[i];
  if (tid < TM_KP) { Gs[tid] = tid < p.K ? p.gamma[tid] : 0.f; Bts[tid] = tid < p.K ? p.beta[tid] : 0.f; }
  if (tid >= 256 && tid < 256 + TM_KP) {
    const int c = tid - 256;
    Scs[c] = (p.c2 && c < p.N) ? p.rs2[(long long)blockIdx.y * p.rs2_ld + c] : 0.f;
    Bps[c] = p.bp[c];
  }

  // ---- att rows -> bf16 fragments -------------------------------------------------------------------------------------------
  bf16x8 xh[TM_KS];
  if (p.io_bf16 & 1) {
    // bf16 att rows (written by the attention kernels' bf16 stores): a lane's fragment of k-step st IS 16 bytes of its token's row
    const long long tk = tok0 + l31 < p.M ? tok0 + l31 : 0;
    const __bf16* arow = reinterpret_cast<const __bf16*>(p.att) + tk * p.lda + 8 * hh;
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
  } else {
    float v[TM_KS][8];
    ff_wave_rows_to_frags<3>(p.att, p.lda, tok0, p.M, p.K, patch, lane, v);
#pragma unroll
    for (int st = 0; st < TM_KS; ++st)
#pragma unroll
      for (int j = 0; j < 8; ++j) xh[st][j] = (__bf16)v[st][j];
  }
  FF_STAMP(64, 1);

  // ---- residual slices: coalesced float4 loads (lane = token row lane>>3 (+8i), channel quad), one slice ahead: slice 0 goes out
  //      right behind the barrier below and lands under the projection's MFMAs, slice n + 1 as soon as slice n has left its registers
  //      for the wave's patch, under slice n's transpose.  ONE register set: a second one (32 registers, c2 may be fp32 here) spills
  //      (hab_link.hip, whose c2 is always bf16, has two).  rc holds
  //      c2 as loaded (bf16 rows: the quad's four bf16 in the first two words, converted -- exactly -- when the slice is consumed), so
  //      that nothing waits for a slice before its turn.
  const int tq = lane >> 3, q4 = 4 * (lane & 7);
  f32x4 rx[4], rc[4];
  // 32-bit element offsets of the lane's four token rows (launcher: M * ld < 2^31); rows past M read row 0 and channels past N
  // read channel 0 instead -- finite values that are never stored and that the zero-padded gamma / beta keep out of fc1
  int xo[4], co[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long tk = tok0 + tq + 8 * i;
    const int t = tk < p.M ? (int)tk : 0;
    xo[i] = t * p.ldx + q4;
    co[i] = t * p.ldc + q4;
  }
  auto load_res = [&](int n) {
    const int cn = (n * 32 + q4 < p.N) ? n * 32 : -q4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rx[i] = *reinterpret_cast<const f32x4*>(p.x + (xo[i] + cn));
      if (p.c2 && (p.io_bf16 & 2)) {
        const f32x2 w2 = *reinterpret_cast<const f32x2*>(reinterpret_cast<const __bf16*>(p.c2) + (co[i] + cn));
        rc[i][0] = w2[0]; rc[i][1] = w2[1];
      } else if (p.c2) rc[i] = *reinterpret_cast<const f32x4*>(p.c2 + (co[i] + cn));
    }
  };
  // vmcnt(0) lgkmcnt(0), as the builtin and not as text: the compiler then knows that nothing is in flight behind it.  After an LDS-DMA
  // it otherwise makes the next use of a loaded register wait for EVERY load issued before that use -- the slices below included
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0x0070);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();                          // the projection image, the vectors and the fragments are in place
  load_res(0);                                           // lands under the projection's MFMAs

#include "token_projmlp_bf16_proj.inc"
  FF_STAMP(64, 2);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                          // every wave is past the projection image: the MLP's first two tiles may land on it
  FF_STAMP(64, 3);
  dma_mlp(0, 0);
  if (p.HT > 1) dma_mlp(1, 1);
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    // x1 = proj + shortcut + conv * scale, slice n: through the wave's patch into accumulator order
    {
      const int c4 = n * 32 + q4;
      const f32x4 sc = *reinterpret_cast<const f32x4*>(Scs + c4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x4 r0 = rx[i];
        f32x4 c2v = rc[i];
        if (p.io_bf16 & 2) {
          const bf16x4 h4 = __builtin_bit_cast(bf16x4, (f32x2){c2v[0], c2v[1]});
          c2v = (f32x4){(float)h4[0], (float)h4[1], (float)h4[2], (float)h4[3]};
        }
        if (p.c2) r0 += c2v * sc;
        *reinterpret_cast<f32x4*>(patch + (tq + 8 * i) * 36 + q4) = r0;
      }
      if (n + 1 < 6) load_res(n + 1);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(patch + l31 * 36 + 8 * g + 4 * hh);
#pragma unroll
        for (int e = 0; e < 4; ++e) oacc[n][4 * g + e] += u[e];
      }
    }
  }
  FF_STAMP(64, 4);

  // ---- LayerNorm(x1) from the accumulators -> fc1 operand --------------------------------------------------------------------
#include "token_projmlp_bf16_ln.inc"
  FF_STAMP(64, 5);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                          // tiles 0 and 1 of the MLP have landed
  FF_STAMP(64, 6);

#define PM_STAMP(i) FF_STAMP(64, i)
#include "token_projmlp_bf16_mlp.inc"
#undef PM_STAMP
  FF_STAMP(64, 40);

  // ---- epilogue: out = accumulators (x1 + fc2 part) + b2, transposed through the wave's patch into 128-byte row segments -----
  {
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      const int c4 = n * 32 + q4;
      const bool cok = c4 < p.N;
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.b2 + (cok ? c4 : 0));
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 v4;
#pragma unroll
        for (int e = 0; e < 4; ++e) v4[e] = oacc[n][4 * g + e];
        *reinterpret_cast<f32x4*>(patch + l31 * 36 + 8 * g + 4 * hh) = v4;
      }
      f32x4 ov[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ov[i] = *reinterpret_cast<const f32x4*>(patch + (tq + 8 * i) * 36 + q4) + b4;
      if (cok) {
        float* op = p.out + (tok0 + tq) * p.ldo + c4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (tok0 + tq + 8 * i < p.M) *reinterpret_cast<f32x4*>(op + (long long)(8 * i) * p.ldo) = ov[i];
      }
    }
  }
  FF_STAMP(64, 41);
  FF_STAMP_DRAINED(64, 42);
}
#undef PM_P

// images == 1: the single-gate launch of ff_token_projmlp, grid (workgroups, 1).  images > 1: grid (workgroups per image, images),
// image b scales c2 by c2_scale + b * scale_ld.
static int token_projmlp_launch(const float* att, int lda, const float* x, int ldx, const float* c2, int ldc, const float* c2_scale,
                                int scale_ld, int images, float* out, int ldo, long long M, int K, int hidden_tiles, const void* proj_tiles,
                                const float* proj_bias_padded, const float* gamma, const float* beta, float eps,
                                const void* mlp_tiles, const float* b1_padded, const float* b2, int nterms, int io_bf16, void* stream) {
  FF_CHECK_ARG(nterms == 1 || nterms == 3, "ff_token_projmlp: nterms must be 1 or 3");
  FF_CHECK_ARG(io_bf16 == 0 || (nterms == 1 && io_bf16 > 0 && io_bf16 < 4), "ff_token_projmlp: bf16 att / c2 rows exist for nterms == 1 only");
  FF_CHECK_ARG(!(io_bf16 & 1) || (lda % 8 == 0 && lda >= ((K + 15) / 16) * 16), "ff_token_projmlp: bf16 att rows must be 16-byte aligned and padded to a multiple of 16 channels");
  FF_CHECK_ARG(att && x && out && proj_tiles && proj_bias_padded && gamma && beta && mlp_tiles && b1_padded && b2, "ff_token_projmlp: null pointer");
  FF_CHECK_ARG(M > 0 && K > 0 && K <= TM_KP && K % 4 == 0 && hidden_tiles > 0, "ff_token_projmlp: needs K <= 192 (K %% 4 == 0)");
  FF_CHECK_ARG(lda >= K && lda % 4 == 0 && ldx >= K && ldx % 4 == 0 && ldo >= K && ldo % 4 == 0, "ff_token_projmlp: rows must be 16-byte aligned");
  FF_CHECK_ARG((((uintptr_t)att) & 15) == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)out) & 15) == 0, "ff_token_projmlp: 16-byte aligned tensors");
  FF_CHECK_ARG((c2 == nullptr) == (c2_scale == nullptr), "ff_token_projmlp: c2 / c2_scale come together");
  FF_CHECK_ARG(!c2 || (ldc >= K && ldc % 4 == 0 && (((uintptr_t)c2) & 15) == 0 && (((uintptr_t)c2_scale) & 15) == 0), "ff_token_projmlp: c2 rows must be 16-byte aligned");
  FF_CHECK_ARG((((uintptr_t)proj_tiles) & 15) == 0 && (((uintptr_t)mlp_tiles) & 15) == 0 && (((uintptr_t)gamma) & 15) == 0 &&
               (((uintptr_t)beta) & 15) == 0 && (((uintptr_t)b2) & 15) == 0, "ff_token_projmlp: weights / gamma / beta / b2 must be 16-byte aligned");
  TokenProjMlpParams p;
  p.att = att; p.x = x; p.c2 = c2; p.rs2 = c2_scale; p.out = out; p.gamma = gamma; p.beta = beta;
  p.wp = (const __bf16*)proj_tiles; p.bp = proj_bias_padded; p.w = (const __bf16*)mlp_tiles; p.b1 = b1_padded; p.b2 = b2;
  p.M = M; p.lda = lda; p.ldx = ldx; p.ldc = ldc; p.ldo = ldo; p.K = K; p.N = K; p.HT = hidden_tiles; p.eps = eps; p.io_bf16 = io_bf16;
  p.wpi = (int)(((M + 255) / 256) / images); p.rs2_ld = images > 1 ? scale_ld : 0;
  FF_STAMP_ARM(p);
  const size_t lds = TM_LDS(hidden_tiles);
  FF_CHECK_ARG(lds <= FF_LDS_MAX, "ff_token_projmlp: hidden too large for the LDS image");
  const long long nblk = (M + 255) / 256;
  const dim3 grid((unsigned)(nblk / images), (unsigned)images);
  FF_CHECK_ARG(nblk < (1LL << 31), "ff_token_projmlp: grid too large");
  FF_CHECK_ARG(M * (long long)(ldx > ldc ? ldx : ldc) < (1LL << 31), "ff_token_projmlp: too many tokens for 32-bit row offsets");
  static ff_device_once once, once2;
  if (!ff_raise_lds(once, "ff_token_projmlp", FF_LDS_MAX, FF_LDS_SAY_ERR, &token_projmlp_kernel)) return FF_ERR_LAUNCH;
  if (nterms == 1) {
    const size_t lds2 = PM_LDS(hidden_tiles);
    FF_CHECK_ARG(lds2 <= FF_LDS_MAX, "ff_token_projmlp: hidden too large for the LDS image");
    if (!ff_raise_lds(once2, "ff_token_projmlp", FF_LDS_MAX, FF_LDS_SAY_ERR, &token_projmlp_bf16_kernel)) return FF_ERR_LAUNCH;
    hipLaunchKernelGGL(token_projmlp_bf16_kernel, grid, dim3(512), lds2, (hipStream_t)stream, p);
  } else hipLaunchKernelGGL(token_projmlp_kernel, grid, dim3(512), lds, (hipStream_t)stream, p);
  FF_LAUNCH_CHECK("ff_token_projmlp");
  return FF_OK;
}

extern "C" int ff_token_projmlp(const float* att, int lda, const float* x, int ldx, const float* c2, int ldc, const float* c2_scale,
                                float* out, int ldo, long long M, int K, int hidden_tiles, const void* proj_tiles,
                                const float* proj_bias_padded, const float* gamma, const float* beta, float eps,
                                const void* mlp_tiles, const float* b1_padded, const float* b2, int nterms, int io_bf16, void* stream) {
  return token_projmlp_launch(att, lda, x, ldx, c2, ldc, c2_scale, 0, 1, out, ldo, M, K, hidden_tiles, proj_tiles, proj_bias_padded, gamma, beta,
                              eps, mlp_tiles, b1_padded, b2, nterms, io_bf16, stream);
}

// ff_token_projmlp over B images of rows_per_image tokens each, with one gate vector per image: c2_scale is [B][scale_ld].  A workgroup owns
// 256 consecutive tokens, so an image must be whole workgroups; B == 1 makes the launch ff_token_projmlp makes.
extern "C" int ff_token_projmlp_images(const float* att, int lda, const float* x, int ldx, const float* c2, int ldc, const float* c2_scale,
                                       int scale_ld, int B, long long rows_per_image, float* out, int ldo, long long M, int K,
                                       int hidden_tiles, const void* proj_tiles, const float* proj_bias_padded, const float* gamma,
                                       const float* beta, float eps, const void* mlp_tiles, const float* b1_padded, const float* b2,
                                       int nterms, int io_bf16, void* stream) {
  FF_CHECK_ARG(B > 0 && B <= 65535 && rows_per_image > 0 && rows_per_image % 256 == 0, "ff_token_projmlp_images: rows_per_image must be a positive multiple of 256 (1 <= B <= 65535)");
  FF_CHECK_ARG(M == (long long)B * rows_per_image, "ff_token_projmlp_images: M must be B * rows_per_image");
  FF_CHECK_ARG(c2 && c2_scale, "ff_token_projmlp_images: the per-image gate needs c2 and c2_scale");
  FF_CHECK_ARG(scale_ld >= K && scale_ld % 4 == 0, "ff_token_projmlp_images: scale_ld must be >= K and a multiple of 4 (16-byte aligned gate rows)");
  return token_projmlp_launch(att, lda, x, ldx, c2, ldc, c2_scale, scale_ld, B, out, ldo, M, K, hidden_tiles, proj_tiles, proj_bias_padded, gamma,
                              beta, eps, mlp_tiles, b1_padded, b2, nterms, io_bf16, stream);
}

extern "C" int ff_token_mlp(const float* x, int ldx, float* out, int ldo, long long M, int K, int hidden_tiles, int N,
                            const float* gamma, const float* beta, float eps, const void* w_tiles, const float* b1_padded,
                            const float* b2, int nterms, void* stream) {
  FF_CHECK_ARG(nterms == 1 || nterms == 3, "ff_token_mlp: nterms must be 1 or 3");
  FF_CHECK_ARG(x && out && gamma && beta && w_tiles && b1_padded && b2, "ff_token_mlp: null pointer");
  FF_CHECK_ARG(M > 0 && K > 0 && K <= TM_KP && K % 4 == 0 && N > 0 && N <= TM_NP && hidden_tiles > 0, "ff_token_mlp: needs K, N <= 192 (K %% 4 == 0)");
  FF_CHECK_ARG(ldx >= K && ldx % 4 == 0 && ldo >= N && (((uintptr_t)x) & 15) == 0, "ff_token_mlp: x rows must be 16-byte aligned");
  FF_CHECK_ARG((((uintptr_t)w_tiles) & 15) == 0 && (((uintptr_t)gamma) & 15) == 0 && (((uintptr_t)beta) & 15) == 0, "ff_token_mlp: weights / gamma / beta must be 16-byte aligned");
  FF_CHECK_ARG(ldx >= N, "ff_token_mlp: the residual is x itself, so N <= ldx");
  TokenMlpParams p;
  p.x = x; p.out = out; p.gamma = gamma; p.beta = beta; p.w = (const __bf16*)w_tiles;
  p.b1 = b1_padded; p.b2 = b2; p.M = M; p.ldx = ldx; p.ldo = ldo; p.K = K; p.N = N; p.HT = hidden_tiles; p.eps = eps;
  const bool vec4 = (N % 4 == 0) && (ldo % 4 == 0) && ((((uintptr_t)out) & 15) == 0) && ((((uintptr_t)b2) & 15) == 0);
  const size_t lds = TM_LDS(hidden_tiles);
  FF_CHECK_ARG(lds <= FF_LDS_MAX, "ff_token_mlp: hidden too large for the LDS image");
  const long long nblk = (M + 255) / 256;
  FF_CHECK_ARG(nblk < (1LL << 31), "ff_token_mlp: grid too large");
#define TM_LAUNCH(V4, NTM)                                                                                                 \
  do {                                                                                                                     \
    static ff_device_once once;                                                                                            \
    if (!ff_raise_lds(once, "ff_token_mlp", FF_LDS_MAX, FF_LDS_SAY_ERR, &token_mlp_kernel<V4, NTM>)) return FF_ERR_LAUNCH; \
    hipLaunchKernelGGL((token_mlp_kernel<V4, NTM>), dim3((unsigned)nblk), dim3(512), lds, (hipStream_t)stream, p);         \
  } while (0)
  if (nterms == 3) { if (vec4) TM_LAUNCH(true, 3); else TM_LAUNCH(false, 3); }
  else { if (vec4) TM_LAUNCH(true, 1); else TM_LAUNCH(false, 1); }
#undef TM_LAUNCH
  FF_LAUNCH_CHECK("ff_token_mlp");
  return FF_OK;
}
