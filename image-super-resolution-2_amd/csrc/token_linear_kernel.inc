// The token-stationary kernel (token_linear.hip includes this file twice).  TL_KERNEL names the kernel; TL_IMAGES = 0 is the kernel of
// ff_token_linear / ff_token_linear_gated.  TL_IMAGES = 1 (GATED): the rows are B images of wpi 256-token workgroups each, the grid is
// (wpi, B), and image blockIdx.y takes its channel gate from row blockIdx.y of cm [B][K] -- a wave-uniform offset that costs no division
// and no vector register.  Nothing else differs.
// TL_OUT16 = 1 (ff_token_linear_rows16; VEC4, no residuals / side outputs): the epilogue multiplies by a per-column scale (p.rs2, kept in
// LDS beside Bs) in fp32 and stores bf16 rows -- p.out is then a __bf16 pointer and p.ldo counts bf16 elements.  The accumulator chain is
// the same text, so a column comes out as bf16(fp32 result * scale).
template <int ACT, int TL_KS, bool VEC4, bool GATED = false, int NTERMS = 3>
__global__ __launch_bounds__(512) void TL_KERNEL(TokenLinParams p) {
  constexpr int TL_SLOTS = 2 * TL_KS + 1, TL_ROWB = TL_SLOTS * 16, TL_PL = 32 * TL_SLOTS, TL_PIECES = 2 * TL_PL / 64;
  constexpr int TL_TILE_ELEMS = 32 * 16 * TL_KS, KPAD = 16 * TL_KS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int BUFB = tl_bufb(TL_KS), WB = BUFB / 2;   // one ring slot (hi + lo planes of WB bytes); the map: lds_layout.h
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  float* tr = reinterpret_cast<float*>(smem + tl_off_tr(TL_KS)) + wid * (32 * TL_TR);   // wave-private transpose patch [token][36]
  float* xs = reinterpret_cast<float*>(smem + tl_off_xs(TL_KS)) + wid * (32 * FF_XS_ROW);   // wave-private x staging
  float* Bs = reinterpret_cast<float*>(smem + tl_off_vec(TL_KS, p.NT, 0));   // [NT*32] bias
#if TL_IMAGES
  const long long tok0 = ((long long)blockIdx.y * p.wpi + blockIdx.x) * 256 + wid * 32;
  const float* cmrow = p.cm + (long long)blockIdx.y * p.K;
#else
  const long long tok0 = (long long)blockIdx.x * 256 + wid * 32;
  const float* cmrow = p.cm;
#endif
  const long long tok = tok0 + l31;
  const bool tvalid = tok < p.M;

  int off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int s = (wid + 8 * i) * 64 + lane;               // slot in the tile image (2 planes x 32 rows x 25 slots)
    if (s >= 2 * TL_PL) s = 2 * TL_PL - 1;
    const int plane = s / TL_PL, t = s - plane * TL_PL, row = t / TL_SLOTS;
    int q = t - row * TL_SLOTS;
    if (q > 2 * TL_KS - 1) q = 2 * TL_KS - 1;
    off[i] = plane * TL_TILE_ELEMS + row * KPAD + q * 8;
  }
  auto dma = [&](int nt, int buf) {
    const __bf16* rec = p.w + (long long)nt * (2 * TL_TILE_ELEMS);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (wid + 8 * i < TL_PIECES)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rec + off[i]),
                                         (__attribute__((address_space(3))) void*)(smem + buf * BUFB + (wid + 8 * i) * 1024), 16, 0, 0);
  };
  dma(0, 0);
  for (int i = tid; i < p.NT * 32; i += 512) Bs[i] = p.bias ? p.bias[i] : 0.f;
#if TL_OUT16
  float* Ss = Bs + p.NT * 32;                        // [NT*32] column scale = tl_off_vec(TL_KS, p.NT, 1), written out: through the function the kernel's scalar code moved
  for (int i = tid; i < p.NT * 32; i += 512) Ss[i] = p.rs2[i];
#endif

  // ---- x rows (+ LayerNorm) -> split bf16 fragments in registers ------------------------------------------------
  bf16x8 xh[TL_KS], xl[TL_KS];
  if constexpr (GATED) {
    // DAT's adaptive interaction folded into the projection's prologue: no pixel-gate kernel, no mix kernel, no 47 MB `fused`
    // tensor.  S = x supplies the per-token gate sm -- its 11-unit first layer is one more 32-row weight tile (index NT of the
    // image, rows 11..31 zero) against S's own fragments -- and takes the per-channel gate cm; O = x2 takes sm.
    dma(p.NT, 1);
    // Two phases, so that at most one set of fragments is live (the one-phase form -- S fragments kept through the O passes and
    // rewritten in place -- needed > 256 registers: 137 dwords of scratch per lane, ~70 MB of spill traffic per launch):
    //   phase 1: S rows -> temporary fragments -> gate GEMM -> sm (one float per lane pair);
    //   phase 2: S and O rows again, 64 channels per pass (S is an L2 hit now), combined in fp32 and split into the final fragments.
    float sm;
    {
      bf16x8 th[TL_KS], tl[TL_KS];
      {
        float v[TL_KS][8];
        ff_wave_rows_to_frags<TL_KS / 4>(p.x, p.ldx, tok0, p.M, p.K, xs, lane, v);
#pragma unroll
        for (int st = 0; st < TL_KS; ++st)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const __bf16 h = (__bf16)v[st][j];
            th[st][j] = h;
            if (NTERMS == 3) tl[st][j] = (__bf16)(v[st][j] - (float)h);
          }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();                                                         // tile 0 (slot 0) and the gate tile (slot 1) landed
      const unsigned char* ap = smem + BUFB + l31 * TL_ROWB + 16 * hh;
      f32x16 ga;
#pragma unroll
      for (int r = 0; r < 16; ++r) ga[r] = p.gb1[(r & 3) + 8 * (r >> 2) + 4 * hh];       // gb1 padded to 32
#define TL_XH th
#define TL_XL tl
#define TL_ACC ga
#include "token_linear_tile_mfma.inc"
#undef TL_XH
#undef TL_XL
#undef TL_ACC
      float sacc = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc += p.gw2[(r & 3) + 8 * (r >> 2) + 4 * hh] * ff_gelu_fast(ga[r]);   // gw2 padded with zeros
      sacc += __shfl_xor(sacc, 32);
      sm = 1.0f / (1.0f + expf(-(sacc + p.gb2)));
    }
    asm volatile("" ::: "memory");
    const int rr = lane >> 4, cq = (lane & 15) * 4;
#pragma unroll
    for (int pass = 0; pass < TL_KS / 4; ++pass) {
      asm volatile("" ::: "memory");                                           // keep the passes apart (no hoisting of all row loads)
      f32x4 tS[8], tO[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = 4 * j + rr, c = 64 * pass + cq;
        const bool ok = tok0 + r < p.M && c < p.K;
        const f32x4 u = *reinterpret_cast<const f32x4*>(p.x + (ok ? (tok0 + r) * p.ldx + c : 0));
        const f32x4 w2 = *reinterpret_cast<const f32x4*>(p.x2 + (ok ? (tok0 + r) * p.ldx2 + c : 0));
        tS[j] = ok ? u : (f32x4){0.f, 0.f, 0.f, 0.f};
        tO[j] = ok ? w2 : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(xs + (4 * j + rr) * FF_XS_ROW + cq) = tS[j];
      f32x4 sa[4], sb[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        sa[s4] = *reinterpret_cast<const f32x4*>(xs + l31 * FF_XS_ROW + 16 * s4 + 8 * hh);
        sb[s4] = *reinterpret_cast<const f32x4*>(xs + l31 * FF_XS_ROW + 16 * s4 + 8 * hh + 4);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(xs + (4 * j + rr) * FF_XS_ROW + cq) = tO[j];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const int st = 4 * pass + s4, k0 = 16 * st + 8 * hh;
        const f32x4 oa = *reinterpret_cast<const f32x4*>(xs + l31 * FF_XS_ROW + 16 * s4 + 8 * hh);
        const f32x4 ob = *reinterpret_cast<const f32x4*>(xs + l31 * FF_XS_ROW + 16 * s4 + 8 * hh + 4);
        const int ka = k0 < p.K ? k0 : 0, kb = k0 + 4 < p.K ? k0 + 4 : 0;
        const f32x4 ca = *reinterpret_cast<const f32x4*>(cmrow + ka), cb = *reinterpret_cast<const f32x4*>(cmrow + kb);
        bf16x8 nh, nl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float o = j < 4 ? oa[j & 3] : ob[j & 3], cmv = j < 4 ? ca[j & 3] : cb[j & 3];
          const float sv = j < 4 ? sa[s4][j & 3] : sb[s4][j & 3];
          const float f = (k0 + j < p.K) ? sv * cmv + o * sm : 0.f;
          const __bf16 h = (__bf16)f;
          nh[j] = h;
          if (NTERMS == 3) nl[j] = (__bf16)(f - (float)h);
        }
        xh[st] = nh;
        if (NTERMS == 3) {
          xl[st] = nl;
          asm volatile("" : "+v"(xh[st]), "+v"(xl[st]) : : "memory");
        } else {
          asm volatile("" : "+v"(xh[st]) : : "memory");
        }            // the pass's fragments are FINISHED here: without this the
      }                                                                        // scheduler issues every pass's loads first and converts last (raw rows of all passes live)
    }
  } else
  {
    float v[TL_KS][8];
    ff_wave_rows_to_frags<TL_KS / 4>(p.x, p.ldx, tok0, p.M, p.K, xs, lane, v);
    float mean = 0.f, rstd = 1.f;
    if (p.gamma) {
      // ff_frag_ln_stats, inline on purpose: with the helper token_linear_kernel<1, 8, false, false, 1> goes from 165 to 169 VGPRs
      // and its reported occupancy from 3 to 2 waves per SIMD (reference and __restrict__ forms alike).  With the statistics epilogue
      // below that form stands at 167 of 168 and <1, 4, true, false, 3> at 128 of 128: the next register costs either a step.
      float s = 0.f;
#pragma unroll
      for (int st = 0; st < TL_KS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[st][j];
      s += __shfl_xor(s, 32);
      mean = s / (float)p.K;
      float qv = 0.f;
#pragma unroll
      for (int st = 0; st < TL_KS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = (16 * st + 8 * hh + j < p.K) ? v[st][j] - mean : 0.f;
          qv += d * d;
        }
      qv += __shfl_xor(qv, 32);
      rstd = 1.0f / sqrtf(qv / (float)p.K + p.eps);
    }
#define LN_OPT_KS TL_KS
#define LN_OPT_TOK tok
#include "frag_ln_opt_step.inc"
#undef LN_OPT_KS
#undef LN_OPT_TOK
  }

  // LayerNorm statistics of a channel range of the (activated) OUTPUT, taken from the accumulators on their way out: the
  // consumer (DAT's SpatialGate: LayerNorm -> depth-wise 3x3, dat_arch.py:117-122) normalises on load, so the separate
  // LayerNorm pass over the 360-channel half (read 94 MB, write 94 MB) disappears
  // Two-pass-grade, although the accumulators leave tile by tile and a second pass does not exist (var = ssq / n - mean^2 from running
  // sums loses rstd digits as (mean / std)^2: 2e-5 relative at 8, 3e-4 at 32).  Every value is first shifted by a pivot, the mean of
  // the lane's first in-range group: where the row's offset is large against its spread the subtraction is exact, and what is left has
  // a mean of about one std at most (a single value as the pivot can be an outlier: it cost the MEAN a digit on GELU rows).  A lane's
  // four activated values of an epilogue group are in registers together, so the group's own mean and centred sum of squares are
  // two-pass; groups merge with the pairwise update (Chan et al.)
  //   n = na + nb, d = mb - ma, m = ma + d nb / n, M2 = M2a + M2b + d^2 na nb / n,
  // which also keeps an outlier pivot harmless.  Two forms that do not do: the pairwise merge without a pivot is first-order in the
  // rounding of every group mean (6e-7 on rstd at mean / std 64, over the bar); a single value as the pivot can be an outlier and
  // costs the mean a digit on GELU rows (2.9e-7 at a bias offset of 0, over its floor of 2^-22).  The running count is a register too: as two scalars (it depends on hh alone) it
  // pushed the non-VEC4 forms past their SGPR budget, and <1, 8, false, false, 1> from 165 to 169 VGPRs.
  float smean = 0.f, sm2 = 0.f, scnt = 0.f, spiv = 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // tile 0 (this wave's DMA pieces) landed
  for (int nt = 0; nt < p.NT; ++nt) {
    const int buf = nt & 1;
    // raw barrier: every wave has waited for its pieces of tile nt (below, before its previous stores) and is done
    // reading ring slot buf^1.  No global-memory ordering is needed across it, so outstanding stores stay in flight.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (nt + 1 < p.NT) dma(nt + 1, buf ^ 1);
    // residuals of this tile are fetched now and consumed after the MFMAs.  vec4 layout (rows 16-byte aligned, N % 4 == 0):
    // lane = (token row tq = lane >> 3 (+8 per step), channel quad cq4 = lane & 7) -> one float4 per lane and step, i.e.
    // 8 whole 128-byte row segments per instruction instead of 2 with dword accesses.
    const int col = nt * 32 + l31;
    const bool cok = col < p.N;
    const int cc = cok ? col : 0;
    const int tq = lane >> 3, c4 = nt * 32 + 4 * (lane & 7);
    const bool c4ok = c4 < p.N;
    float rv[16];
    f32x4 rq[4];
    if (VEC4 && !TL_OUT16) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long tk = tok0 + tq + 8 * i;
        const bool ok = c4ok && tk < p.M;
        f32x4 r0 = {0.f, 0.f, 0.f, 0.f};
        if (p.res) { const f32x4 u = *reinterpret_cast<const f32x4*>(p.res + (ok ? tk * p.ldr + c4 : 0)); r0 = ok ? u : r0; }
        if (p.res2) {
          const f32x4 u = *reinterpret_cast<const f32x4*>(p.res2 + (ok ? tk * p.ldr2 + c4 : 0));
          const f32x4 sc = *reinterpret_cast<const f32x4*>(p.rs2 + (c4ok ? c4 : 0));
          if (ok) r0 += u * sc;
        }
        rq[i] = r0;
      }
    } else if (!VEC4) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const long long tk = tok0 + 2 * i + hh;
        const long long tqq = tk < p.M ? tk : 0;
        float r0 = p.res ? p.res[tqq * p.ldr + cc] : 0.f;
        if (p.res2) r0 += p.res2[tqq * p.ldr2 + cc] * p.rs2[cc];
        rv[i] = r0;
      }
    }
    const unsigned char* ap = smem + buf * BUFB + l31 * TL_ROWB + 16 * hh;
    f32x16 acc;
    {
      const int nb = nt * 32 + 4 * hh;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = Bs[nb + (r & 3) + 8 * (r >> 2)];
    }
#define TL_XH xh
#define TL_XL xl
#define TL_ACC acc
#include "token_linear_tile_mfma.inc"
#undef TL_XH
#undef TL_XL
#undef TL_ACC
    // ---- epilogue of this tile: act, transpose through the wave's LDS patch, coalesced row-segment stores --------
    // accumulator register r of lane (l31 = token, hh) is channel (r & 3) + 8 (r >> 2) + 4 hh: four consecutive channels
    // per r >> 2 -> one ds_write_b128 each
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 v4;
      if (ACT == ACT_GELU && NTERMS == 1 && TL_GELU_SIG) {      // plain bf16: the sigmoid form (ff_common.h)
        const f32x2 ga = ff_gelu_sig2((f32x2){acc[4 * g], acc[4 * g + 1]}), gb = ff_gelu_sig2((f32x2){acc[4 * g + 2], acc[4 * g + 3]});
        v4 = (f32x4){ga[0], ga[1], gb[0], gb[1]};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v4[e] = ff_act_c<ACT, true>(acc[4 * g + e]);
      }
      *reinterpret_cast<f32x4*>(tr + l31 * TL_TR + 8 * g + 4 * hh) = v4;
      if (!TL_OUT16 && p.stats && nt * 32 + 8 * g + 8 > p.st_lo && nt * 32 + 8 * g < p.st_hi) {      // wave-uniform: the group meets the range
        const int cb = nt * 32 + 8 * g + 4 * hh;
        const float cn = (float)max(0, min(cb + 4, p.st_hi) - max(cb, p.st_lo));
        float w[4], ts = 0.f, tq2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          w[e] = (cb + e >= p.st_lo && cb + e < p.st_hi) ? v4[e] - spiv : 0.f;
          ts += w[e];
        }
        float tm = ts * __builtin_amdgcn_rcpf(fmaxf(cn, 1.f));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = (cb + e >= p.st_lo && cb + e < p.st_hi) ? w[e] - tm : 0.f;
          tq2 += d * d;
        }
        const bool first = scnt == 0.f;            // the lane's first in-range group: spiv was 0, so tm is the group's plain mean --
        spiv = first ? tm : spiv;                  // it becomes the pivot, and the group's shifted mean is 0 (no branch: a divergent
        tm = first ? 0.f : tm;                     // one cost <1, 4, true, false, 3> and <1, 8, false, false, 1> an occupancy step)
        const float dl = tm - smean, wn = cn * __builtin_amdgcn_rcpf(fmaxf(scnt + cn, 1.f));   // cn = 0: nothing moves
        smean += dl * wn;
        sm2 += tq2 + dl * dl * scnt * wn;
        scnt += cn;
      }
    }
    // One wait per tile, placed BEFORE this tile's stores: it retires the DMA of tile nt+1 (issued a whole tile ago),
    // this tile's residual loads and the PREVIOUS tile's stores -- so stores always have a full tile to drain
    // (vmcnt counts stores too; waiting right after issuing them would serialise the kernel on HBM write latency).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#if TL_OUT16
    {
      const f32x4 cs = *reinterpret_cast<const f32x4*>(Ss + nt * 32 + 4 * (lane & 7));
      bf16x4 ov[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 t4 = *reinterpret_cast<const f32x4*>(tr + (tq + 8 * i) * TL_TR + 4 * (lane & 7)) * cs;
        ov[i] = (bf16x4){(__bf16)t4[0], (__bf16)t4[1], (__bf16)t4[2], (__bf16)t4[3]};
      }
      if (c4ok) {
        __bf16* op = reinterpret_cast<__bf16*>(p.out) + (tok0 + tq) * p.ldo + c4;
        if (tok0 + 32 <= p.M) {
#pragma unroll
          for (int i = 0; i < 4; ++i) *reinterpret_cast<bf16x4*>(op + (long long)(8 * i) * p.ldo) = ov[i];
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (tok0 + tq + 8 * i < p.M) *reinterpret_cast<bf16x4*>(op + (long long)(8 * i) * p.ldo) = ov[i];
        }
      }
    }
#else
    if (VEC4) {
      f32x4 ov[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ov[i] = *reinterpret_cast<const f32x4*>(tr + (tq + 8 * i) * TL_TR + 4 * (lane & 7)) + rq[i];
      if (c4ok) {
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
    } else {
      float ov[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) ov[i] = tr[(2 * i + hh) * TL_TR + l31] + rv[i];      // 16 LDS reads back to back
      if (cok) {                                                                        // one exec mask for the whole tile
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
#endif
  }
  if (!TL_OUT16 && p.stats) {                                              // (the rows16 entry point takes no statistics output)
    // the lane pair (l, l ^ 32) holds the two halves of the token's range: one more pairwise merge, still in the shifted domain (the
    // pivots' difference is exact where it matters), written by the hh = 0 lane
    const float na = scnt, nb = __shfl_xor(scnt, 32);
    const float mo = __shfl_xor(smean, 32), m2o = __shfl_xor(sm2, 32), po = __shfl_xor(spiv, 32);
    const float n = fmaxf(na + nb, 1.f), dl = (nb > 0.f && na > 0.f) ? (po - spiv) + (mo - smean) : 0.f;
    const float mean = (na > 0.f ? spiv + (smean + dl * (nb / n)) : po + mo);
    const float var = (sm2 + m2o + dl * dl * (na * nb / n)) / n;
    if (hh == 0 && tvalid) *reinterpret_cast<float2*>(p.stats + 2 * tok) = make_float2(mean, 1.0f / sqrtf(var + p.st_eps));
  }
}
