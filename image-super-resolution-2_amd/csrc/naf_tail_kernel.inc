// The NAFBlock tail kernel (naf_tail.hip includes this file twice).  NAF_TAIL_KERNEL names the kernel; NAF_TAIL_IMG = 0 is the single-image
// form, whose text is exactly what the preprocessor leaves of this file with the IMG parts removed.
// NAF_TAIL_IMG = 1: conv3's A-operand scale comes from sca[image][C], image = tok0 / rpi recomputed per tile (the persistent tile loop
// walks across image boundaries).  B vectors do not fit in LDS next to the weights, ONE PER WAVE does (NW * C floats): a wave fetches
// its image's vector with the g / x rows of the tile (one or two dwords per lane, an L2 hit, in flight under the previous tile), drops
// it into its own LDS slot at the top of the tile and reads s0 / s1 there as the single-image form reads the constant block --
// wave-private, so no barrier, and no registers held through the tile (reading the vector from global memory in place spilled at
// c = 64).  Everything else -- and with it every rounding -- is the single-image body.
#if NAF_TAIL_IMG
#define NAF_TAIL_SCA scw
#else
#define NAF_TAIL_SCA cs
#endif
template <int KS, int NW>
__global__ __launch_bounds__(NW * 64, (KS == 4 ? 2 : 1)) void NAF_TAIL_KERNEL(NafTailParams p) {
  constexpr int C = 16 * KS, GT = C / 32, NTO = C / 32;
  constexpr int NT = NW * 64;
  // row gather: CPP channels per pass.  64 at c = 64 (whole 256-byte rows, four per load instruction); 32 at c = 128 (eight
  // 128-byte segments per instruction) -- the patch is then 4.5 KB per wave and FOUR waves fit next to the 128 KB of weights
  constexpr int CPP = KS == 4 ? 64 : 32, NPASS = C / CPP, XROW = ntl_xrow(KS);   // patch row: CPP + 4 dwords = 4 (mod 32): conflict-free b128 (the map: lds_layout.h)
  constexpr int LPR = CPP / 4, RPI = 64 / LPR, LPP = 32 / RPI, FPP = CPP / 16;   // lanes per row, rows per instruction, loads / fragments per pass
  constexpr bool EARLY = KS == 8;                      // c = 128 (one wave per SIMD, 512 registers): next tile's loads in flight during conv3 too
  constexpr int WPIECES = 4 * C * C / 8;               // 16-byte pieces of the weight image
  constexpr int F4 = NTO * KS, F5 = F4 + 2 * GT * KS;  // first fragment of W4 / W5
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const bf16x8* Wl = reinterpret_cast<const bf16x8*>(smem);            // [fragment][64 lanes]
  float* cs = reinterpret_cast<float*>(smem + ntl_off_cs(KS));          // sca | b3 | beta | ln_g | ln_b | b4 (2C) | b5 | gamma
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: scalar row bases
  const int l31 = lane & 31, hh = lane >> 5;
  const int rr = lane / LPR, cq = (lane % LPR) * 4;
  float* xs = reinterpret_cast<float*>(smem + ntl_off_xs(KS)) + wid * (32 * XROW);   // wave-private patch: row gather, later the 32 x 33 transposes
  static_assert(33 <= XROW, "the 32 x 33 transpose must fit in the wave's gather patch");
#if NAF_TAIL_IMG
  float* scw = reinterpret_cast<float*>(smem + ntl_off_sca(KS, NW)) + wid * C;   // the wave's slot for its image's sca vector
  float nsca[C / 64];                                                   // the next tile's vector, lane l holds channels l (+ 64)
#endif

  // the wave's g and x rows of one tile in registers: whole 128-byte lines, RPI rows per load instruction
  f32x4 tg[NPASS][LPP], tx[NPASS][LPP];
  const unsigned og = (unsigned)(rr * p.ldg + cq), ox = (unsigned)(rr * p.ldx + cq);      // lane offsets inside an RPI-row group
  auto issue = [&](long long tok0) {
#if NAF_TAIL_IMG
    {                                                    // (a wave past the last row computes on zeros and stores nothing: clamp its image)
      unsigned im = (unsigned)tok0 / (unsigned)p.rpi;
      if (im >= (unsigned)p.nimg) im = (unsigned)p.nimg - 1u;
      const float* sp = p.sca + (size_t)__builtin_amdgcn_readfirstlane(im) * C + lane;
#pragma unroll
      for (int j = 0; j < C / 64; ++j) nsca[j] = sp[64 * j];
    }
#endif
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
#if NAF_TAIL_IMG
#pragma unroll
    for (int j = 0; j < C / 64; ++j) scw[64 * j + lane] = nsca[j];
#endif
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
#pragma unroll
      for (int j = 0; j < LPP; ++j) *reinterpret_cast<f32x4*>(xs + (RPI * j + rr) * XROW + cq) = tg[pass][j];
#pragma unroll
      for (int s4 = 0; s4 < FPP; ++s4) {
        const int st = FPP * pass + s4, k0 = 16 * st + 8 * hh;
        const f32x4 a = *reinterpret_cast<const f32x4*>(xs + l31 * XROW + 16 * s4 + 8 * hh);
        const f32x4 b = *reinterpret_cast<const f32x4*>(xs + l31 * XROW + 16 * s4 + 8 * hh + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(NAF_TAIL_SCA + k0), s1 = *reinterpret_cast<const f32x4*>(NAF_TAIL_SCA + k0 + 4);
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
#include "naf_ln_stats.inc"
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
#undef NAF_TAIL_SCA
