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
};

template <int KS, int NW>
__global__ __launch_bounds__(NW * 64, (KS == 4 ? 2 : 1)) void naf_tail_kernel(NafTailParams p) {
  constexpr int C = 16 * KS, GT = C / 32, NTO = C / 32;
  constexpr int NT = NW * 64;
  // row gather: CPP channels per pass.  64 at c = 64 (whole 256-byte rows, four per load instruction); 32 at c = 128 (eight
  // 128-byte segments per instruction) -- the patch is then 4.5 KB per wave and FOUR waves fit next to the 128 KB of weights
  constexpr int CPP = KS == 4 ? 64 : 32, NPASS = C / CPP, XROW = CPP + 4;   // patch row: CPP + 4 dwords = 4 (mod 32): conflict-free b128
  constexpr int LPR = CPP / 4, RPI = 64 / LPR, LPP = 32 / RPI, FPP = CPP / 16;   // lanes per row, rows per instruction, loads / fragments per pass
  constexpr bool EARLY = KS == 8;                      // c = 128 (one wave per SIMD, 512 registers): next tile's loads in flight during conv3 too
  constexpr int WPIECES = 4 * C * C / 8;               // 16-byte pieces of the weight image
  constexpr int F4 = NTO * KS, F5 = F4 + 2 * GT * KS;  // first fragment of W4 / W5
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const bf16x8* Wl = reinterpret_cast<const bf16x8*>(smem);            // [fragment][64 lanes]
  float* cs = reinterpret_cast<float*>(smem + 8 * C * C);               // sca | b3 | beta | ln_g | ln_b | b4 (2C) | b5 | gamma
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: scalar row bases
  const int l31 = lane & 31, hh = lane >> 5;
  const int rr = lane / LPR, cq = (lane % LPR) * 4;
  float* xs = cs + 9 * C + wid * (32 * XROW);                           // wave-private patch: row gather, later the 32 x 33 transposes

  // the wave's g and x rows of one tile in registers: whole 128-byte lines, RPI rows per load instruction
  f32x4 tg[NPASS][LPP], tx[NPASS][LPP];
  const unsigned og = (unsigned)(rr * p.ldg + cq), ox = (unsigned)(rr * p.ldx + cq);      // lane offsets inside an RPI-row group
  auto issue = [&](long long tok0) {
    const float* gp = p.g + tok0 * p.ldg;
    const float* xp = p.x + tok0 * p.ldx;
    if (tok0 + 32 <= p.M) {                              // whole tile in range: scalar row bases, one lane offset per tensor
#pragma unroll
      for (int pass = 0; pass < NPASS; ++pass)
#pragma unroll
        for (int j = 0; j < LPP; ++j) {
          tg[pass][j] = *reinterpret_cast<const f32x4*>(gp + (long long)(RPI * j) * p.ldg + CPP * pass + og);
          tx[pass][j] = *reinterpret_cast<const f32x4*>(xp + (long long)(RPI * j) * p.ldx + CPP * pass + ox);
        }
    } else {
#pragma unroll
      for (int pass = 0; pass < NPASS; ++pass)
#pragma unroll
        for (int j = 0; j < LPP; ++j) {
          const bool ok = tok0 + RPI * j + rr < p.M;
          const f32x4 a = *reinterpret_cast<const f32x4*>(ok ? gp + (long long)(RPI * j) * p.ldg + CPP * pass + og : p.g);
          const f32x4 b = *reinterpret_cast<const f32x4*>(ok ? xp + (long long)(RPI * j) * p.ldx + CPP * pass + ox : p.x);
          tg[pass][j] = ok ? a : (f32x4){0.f, 0.f, 0.f, 0.f};
          tx[pass][j] = ok ? b : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
  };
  long long tile = blockIdx.x;
  issue((tile * NW + wid) * 32);

  for (int i = tid; i < WPIECES; i += NT) reinterpret_cast<uint4*>(smem)[i] = reinterpret_cast<const uint4*>(p.w)[i];
  for (int i = tid; i < C; i += NT) {
    cs[i] = p.sca[i]; cs[C + i] = p.b3[i]; cs[2 * C + i] = p.beta[i]; cs[3 * C + i] = p.gamma_ln[i]; cs[4 * C + i] = p.beta_ln[i];
    cs[5 * C + i] = p.b4[i]; cs[6 * C + i] = p.b4[C + i]; cs[7 * C + i] = p.b5[i]; cs[8 * C + i] = p.oscale[i];
  }
  __syncthreads();

  for (; tile < p.ntiles; tile += gridDim.x) {
    const long long tok0 = (tile * NW + wid) * 32;
    // ---- rows -> MFMA B-operand order through the patch: v[st][j] = row l31, channel 16 st + 8 hh + j ------------------
    bf16x8 gb[KS];
    float v[KS][8];
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
#pragma unroll
      for (int j = 0; j < LPP; ++j) *reinterpret_cast<f32x4*>(xs + (RPI * j + rr) * XROW + cq) = tg[pass][j];
#pragma unroll
      for (int s4 = 0; s4 < FPP; ++s4) {
        const int st = FPP * pass + s4, k0 = 16 * st + 8 * hh;
        const f32x4 a = *reinterpret_cast<const f32x4*>(xs + l31 * XROW + 16 * s4 + 8 * hh);
        const f32x4 b = *reinterpret_cast<const f32x4*>(xs + l31 * XROW + 16 * s4 + 8 * hh + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(cs + k0), s1 = *reinterpret_cast<const f32x4*>(cs + k0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { gb[st][e] = (__bf16)(a[e] * s0[e]); gb[st][4 + e] = (__bf16)(b[e] * s1[e]); }
      }
    }
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
#pragma unroll
      for (int j = 0; j < LPP; ++j) *reinterpret_cast<f32x4*>(xs + (RPI * j + rr) * XROW + cq) = tx[pass][j];
#pragma unroll
      for (int s4 = 0; s4 < FPP; ++s4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(xs + l31 * XROW + 16 * s4 + 8 * hh);
        const f32x4 b = *reinterpret_cast<const f32x4*>(xs + l31 * XROW + 16 * s4 + 8 * hh + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[FPP * pass + s4][e] = a[e]; v[FPP * pass + s4][4 + e] = b[e]; }
      }
    }
    if (EARLY && tile + gridDim.x < p.ntiles) issue(((tile + gridDim.x) * NW + wid) * 32);

    // ---- conv3: Y^T tiles (A = W3 rows, B = the scaled gate), epilogue values into the row-gather layout, + x -----------
#pragma unroll
    for (int n = 0; n < NTO; ++n) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int st = 0; st < KS; ++st) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wl[(n * KS + st) * 64 + lane], gb[st], acc, 0, 0, 0);
      unsigned tt[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = 32 * n + (r & 3) + 8 * (r >> 2) + 4 * hh;
        tt[r] = __float_as_uint((acc[r] + cs[C + ch]) * cs[2 * C + ch]);
      }
      // registers 4q + e hold channel 8q + 4hh + e; the swap hands the upper half-wave's even q to the lower half-wave and the
      // lower one's odd q to the upper: afterwards {even, odd} = channels 16sp + 8hh + {e, 4 + e}
#pragma unroll
      for (int sp = 0; sp < 2; ++sp)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const auto sw = __builtin_amdgcn_permlane32_swap(tt[8 * sp + e], tt[8 * sp + 4 + e], false, false);
          v[2 * n + sp][e] = __uint_as_float(sw[0]) + v[2 * n + sp][e];
          v[2 * n + sp][4 + e] = __uint_as_float(sw[1]) + v[2 * n + sp][4 + e];
        }
    }

    // c = 64 (two waves per SIMD, 256 registers): the next tile's loads start here, in flight during the gated FFN and the stores
    if (!EARLY && tile + gridDim.x < p.ntiles) issue(((tile + gridDim.x) * NW + wid) * 32);

    // ---- from here on naf_ffn_kernel<KS, 1> with y = v: LayerNorm2d, the sums in the gather's order -----------------------
    bf16x8 xh[KS];
    {
      // the LayerNorm of ff_common.h (ff_frag_ln_stats / _step), inline on purpose: through the helpers naf_tail_kernel<8, 4> goes
      // from 202 to 214 AGPRs and from 110.94 / 110.39 us to 112.22 / 111.89 us under the bench
      float s = 0.f;
#pragma unroll
      for (int st = 0; st < KS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[st][j];
      s += __shfl_xor(s, 32);
      const float mean = s / (float)C;
      float qv = 0.f;
#pragma unroll
      for (int st = 0; st < KS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[st][j] - mean; qv += d * d; }
      qv += __shfl_xor(qv, 32);
      const float rstd = 1.0f / sqrtf(qv / (float)C + p.eps);
#pragma unroll
      for (int st = 0; st < KS; ++st) {
        const int k0 = 16 * st + 8 * hh;
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(cs + 3 * C + k0), g1 = *reinterpret_cast<const f32x4*>(cs + 3 * C + k0 + 4);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(cs + 4 * C + k0), b1 = *reinterpret_cast<const f32x4*>(cs + 4 * C + k0 + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = (v[st][j] - mean) * rstd * (j < 4 ? g0[j & 3] : g1[j & 3]) + (j < 4 ? b0[j & 3] : b1[j & 3]);
          xh[st][j] = (__bf16)f;
        }
      }
    }

    f32x16 oacc[NTO];
#pragma unroll
    for (int n = 0; n < NTO; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[n][r] = 0.f;

#pragma unroll
    for (int g = 0; g < GT; ++g) {
      // two H^T tiles: channels [32g, 32g+32) and [C + 32g, C + 32g + 32) of conv4
      f32x16 ha, hb;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = 32 * g + (r & 3) + 8 * (r >> 2) + 4 * hh;
        ha[r] = cs[5 * C + ch];
        hb[r] = cs[6 * C + ch];
      }
#pragma unroll
      for (int st = 0; st < KS; ++st) {
        ha = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wl[(F4 + (2 * g) * KS + st) * 64 + lane], xh[st], ha, 0, 0, 0);
        hb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wl[(F4 + (2 * g + 1) * KS + st) * 64 + lane], xh[st], hb, 0, 0, 0);
      }
      // SimpleGate: product of the two tiles; registers 8s..8s+7 are the B fragment of k-step s (W5's columns are permuted to match)
      bf16x8 gh[2];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) gh[s][j] = (__bf16)(ha[8 * s + j] * hb[8 * s + j]);
#pragma unroll
      for (int n = 0; n < NTO; ++n)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          oacc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Wl[(F5 + (g * NTO + n) * 2 + s) * 64 + lane], gh[s], oacc[n], 0, 0, 0);
    }

    // ---- epilogue: out = y + gamma[n] * (acc + b5[n]); the y tile, then the accumulator tile, transposed through the patch ----
    float* tr = xs;
#pragma unroll
    for (int n = 0; n < NTO; ++n) {
#pragma unroll
      for (int sp = 0; sp < 2; ++sp)
#pragma unroll
        for (int j = 0; j < 8; ++j) tr[l31 * 33 + 16 * sp + 8 * hh + j] = v[2 * n + sp][j];
      float rv[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) rv[i] = tr[(2 * i + hh) * 33 + l31];
#pragma unroll
      for (int r = 0; r < 16; ++r) tr[l31 * 33 + (r & 3) + 8 * (r >> 2) + 4 * hh] = oacc[n][r];
      const int col = n * 32 + l31;
      const float sc = cs[8 * C + col], bb = cs[7 * C + col];
      float ov[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) ov[i] = (tr[(2 * i + hh) * 33 + l31] + bb) * sc + rv[i];
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

// hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage:
//   kernel            VGPRs  AGPRs  scratch  LDS (dynamic)  waves/SIMD  workgroups/CU
//   naf_tail<4, 4>    252    0      0        69 888 B       2           2  (c = 64: 8 waves per CU)
//   naf_tail<8, 4>    256    202    0        154 112 B      1           1  (c = 128: 4 waves per CU)
template <int KS, int NW, int WGPC>
static int launch_naf_tail(NafTailParams& p, hipStream_t st) {
  constexpr int C = 16 * KS;
  constexpr size_t lds = (size_t)8 * C * C + (size_t)9 * C * 4 + (size_t)NW * 32 * ((KS == 4 ? 64 : 32) + 4) * 4;
  static_assert(lds <= 160 * 1024, "LDS budget");
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&naf_tail_kernel<KS, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { ff_set_error("ff_naf_tail: cannot raise dynamic LDS: %s", hipGetErrorString(e)); return FF_ERR_LAUNCH; }
    attr_set = true;
  }
  const long long ntiles = (p.M + NW * 32 - 1) / (NW * 32);
  if (ntiles >= (1LL << 31)) { ff_set_error("ff_naf_tail: too many rows"); return FF_ERR_ARG; }
  p.ntiles = (int)ntiles;
  const long long nblk = ntiles < 256 * WGPC ? ntiles : 256 * WGPC;      // persistent: WGPC workgroups per CU stride over the tiles
  hipLaunchKernelGGL((naf_tail_kernel<KS, NW>), dim3((unsigned)nblk), dim3(NW * 64), lds, st, p);
  FF_LAUNCH_CHECK("ff_naf_tail");
  return FF_OK;
}

extern "C" int ff_naf_tail(const float* g, int ldg, const float* x, int ldx, float* out, int ldo, long long M, int C,
                           const float* sca, const float* b3, const float* beta, const float* gamma_ln, const float* beta_ln,
                           float eps, const void* w_frags, const float* b4, const float* b5, const float* out_scale, void* stream) {
  FF_CHECK_ARG(g && x && out && sca && b3 && beta && gamma_ln && beta_ln && w_frags && b4 && b5 && out_scale, "ff_naf_tail: null pointer");
  FF_CHECK_ARG(M > 0 && (C == 64 || C == 128), "ff_naf_tail: C must be 64 or 128");
  FF_CHECK_ARG(ldg >= C && ldg % 4 == 0 && ldx >= C && ldx % 4 == 0 && ldo >= C, "ff_naf_tail: row strides must be >= C (g, x: multiples of 4)");
  FF_CHECK_ARG((((uintptr_t)g) & 15) == 0 && (((uintptr_t)x) & 15) == 0 && (((uintptr_t)w_frags) & 15) == 0, "ff_naf_tail: 16-byte alignment required");
  FF_CHECK_ARG(out != g && out != x, "ff_naf_tail: out must not alias g or x");
  NafTailParams p;
  p.g = g; p.x = x; p.out = out; p.w = (const __bf16*)w_frags; p.sca = sca; p.b3 = b3; p.beta = beta; p.gamma_ln = gamma_ln;
  p.beta_ln = beta_ln; p.b4 = b4; p.b5 = b5; p.oscale = out_scale; p.M = M; p.ldg = ldg; p.ldx = ldx; p.ldo = ldo; p.eps = eps;
  p.ntiles = 0;
  return C == 64 ? launch_naf_tail<4, 4, 2>(p, (hipStream_t)stream) : launch_naf_tail<8, 4, 1>(p, (hipStream_t)stream);
}
