// The NAFBlock front kernel (naf_front.inc includes this file twice).  NF_KERNEL names the kernel; NF_IMAGES = 0 is the single-image form,
// NF_IMAGES = 1 the form for B images in one launch, grid (tiles, B): the image is blockIdx.y, while blockIdx.x, its XCD remap and the
// partial row it writes are those of the image's own launch.
template <int KS, int NTERMS>
__global__ __launch_bounds__(512, KS == 4 ? 4 : 2) void NF_KERNEL(NafFrontParams p) {   // C = 64: two workgroups per CU (70 KB of LDS each)
  constexpr int C = 16 * KS, NCH = C / 32;                      // channels, gated 32-channel chunks
  constexpr int WROWB = 4 * C + 16;                             // LDS weight row: [C hi | C lo | 16 B pad]
  constexpr int WTILEB = nfr_wtileb(C);                         // the map: lds_layout.h
  constexpr int ITEMS = 32 * C * 2 * 2 / 16;                    // 16-byte items per weight tile (hi + lo)
  constexpr int IPT = (2 * ITEMS + 511) / 512;                  // items per thread for the two tiles of a chunk
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Tt = reinterpret_cast<float*>(smem);                   // [192][NF_TS]: phase 0 row staging, then the conv1 output tile
  unsigned char* Ws = smem + nfr_off_w();                       // [2 tiles][32][WROWB]
  float* red = reinterpret_cast<float*>(smem + nfr_off_red(C)); // [8 waves][8 quads][4]
  float* Wd = reinterpret_cast<float*>(smem + nfr_off_wd(C));   // [9][2C] depth-wise taps, [2C] depth-wise bias, [2C] conv1 bias

#if NF_IMAGES
  {                                                              // image blockIdx.y: its pixels, and its rows of part [B][tiles][C]
    const long long b = blockIdx.y, P = (long long)p.H * p.W;
    p.x += b * P * p.ldx;
    p.out += b * P * p.ldo;
    p.part += b * ((long long)p.tiles_x * p.tiles_y) * (16 * KS);
  }
#endif
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int L = ff_xcd_remap(blockIdx.x, p.tiles_x * p.tiles_y);
  const int x0 = (L % p.tiles_x) * NF_TX, y0 = (L / p.tiles_x) * NF_TY;

  // ---- weight tiles of a chunk: global -> registers -> LDS (two 32-row tiles: channels 32 jc.. and C + 32 jc..) --------------
  uint4 wreg[IPT];
  auto wload = [&](int jc) {
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const int id = tid + 512 * i;                             // [tile][plane][row][C/8 items]
      uint4 v = {0u, 0u, 0u, 0u};
      if (id < 2 * ITEMS) {
        const int tile = id / ITEMS, rem = id - tile * ITEMS;
        const int nt = tile == 0 ? jc : NCH + jc;
        v = *reinterpret_cast<const uint4*>(p.w1 + (long long)nt * (2 * 32 * C) + rem * 8);
      }
      wreg[i] = v;
    }
  };
  auto wstore = [&]() {
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
      const int id = tid + 512 * i;
      if (id < 2 * ITEMS) {
        const int tile = id / ITEMS, rem = id - tile * ITEMS;
        const int plane = rem / (32 * C / 8), r2 = rem - plane * (32 * C / 8);
        const int row = r2 / (C / 8), q = r2 - row * (C / 8);
        *reinterpret_cast<uint4*>(Ws + tile * WTILEB + row * WROWB + plane * 2 * C + q * 16) = wreg[i];
      }
    }
  };
  wload(0);
  for (int i = tid; i < 11 * 2 * C; i += 512)                    // (visible after the barrier that closes phase 0)
    Wd[i] = i < 9 * 2 * C ? p.wdw[i] : (i < 10 * 2 * C ? p.bdw[i - 9 * 2 * C] : p.b1[i - 10 * 2 * C]);

  // ---- phase 0: this wave's 32 halo tokens -> LayerNorm -> split-bf16 fragments (waves 0..5) ---------------------------------
  bf16x8 xh[KS], xl[KS];
  const int tokw = wid * 32 + l31;                               // halo token of this lane in fragment / accumulator order
  bool tvalid = false;
  if (wid < NF_MT) {
    const int hy = tokw / NF_HW, hx = tokw - hy * NF_HW;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    tvalid = tokw < NF_NTOK && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    float* xs = Tt + wid * 32 * NF_TS;                           // the wave's own 32 rows of the tile buffer
    const int rr = lane >> 4, cq = (lane & 15) * 4;
    int roff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int t = wid * 32 + 4 * j + rr;
      const int ty = t / NF_HW, tx = t - ty * NF_HW;
      const int yy = y0 - 1 + ty, xx = x0 - 1 + tx;
      const bool ok = t < NF_NTOK && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
      roff[j] = ok ? ((ty - 1) * p.W + (tx - 1)) * p.ldx : NF_BAD;       // relative to the tile's first pixel (64-bit base below)
    }
    const float* xb = p.x + ((long long)y0 * p.W + x0) * p.ldx;     // wave-uniform 64-bit base: 8160 x 5424 x 64 floats exceed 31 bits
    float v[KS][8];
#pragma unroll
    for (int pass = 0; pass < KS / 4; ++pass) {
      f32x4 t4[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = roff[j] != NF_BAD;
        const f32x4 u = *reinterpret_cast<const f32x4*>(ok ? xb + (roff[j] + 64 * pass + cq) : p.x);
        t4[j] = ok ? u : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(xs + (4 * j + rr) * NF_TS + cq) = t4[j];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(xs + l31 * NF_TS + 16 * s4 + 8 * hh);
        const f32x4 b = *reinterpret_cast<const f32x4*>(xs + l31 * NF_TS + 16 * s4 + 8 * hh + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[4 * pass + s4][e] = a[e]; v[4 * pass + s4][4 + e] = b[e]; }
      }
    }
    // the LayerNorm of ff_common.h (ff_frag_ln_stats / _step / ff_bf16_split), inline on purpose: through the helpers
    // naf_front_kernel<4, 1> measured 293.2 / 279.3 us against 278.8 / 272.5 us under the bench
#include "naf_ln_stats.inc"
#pragma unroll
    for (int st = 0; st < KS; ++st) {
      const int k0 = 16 * st + 8 * hh;
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(p.gamma + k0), g1 = *reinterpret_cast<const f32x4*>(p.gamma + k0 + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.beta + k0), b1v = *reinterpret_cast<const f32x4*>(p.beta + k0 + 4);
      bf16x8 nh, nl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (v[st][j] - mean) * rstd * (j < 4 ? g0[j & 3] : g1[j & 3]) + (j < 4 ? b0[j & 3] : b1v[j & 3]);
        const __bf16 h = (__bf16)f;
        nh[j] = h;
        nl[j] = (__bf16)(f - (float)h);
      }
      xh[st] = nh;
      xl[st] = nl;
    }
  }
  wstore();
  __syncthreads();                                               // weights of chunk 0 in LDS; every wave is done with its staging rows

  const int c4 = tid & 7;                                        // depth-wise phase: channel quad of the chunk, two pixels per thread
  for (int jc = 0; jc < NCH; ++jc) {
    // ---- conv1, two 32-channel tiles, into the LDS tile (zeros outside the image) --------------------------------------------
    if (wid < NF_MT) {
#pragma unroll
      for (int tile = 0; tile < 2; ++tile) {
        const unsigned char* ap = Ws + tile * WTILEB + l31 * WROWB + 16 * hh;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int st = 0; st < KS; ++st) {
          const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ap + 32 * st);
          const bf16x8 al = *reinterpret_cast<const bf16x8*>(ap + 32 * st + 2 * C);
          if (NTERMS == 3) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xl[st], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, xh[st], acc, 0, 0, 0);
          }
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xh[st], acc, 0, 0, 0);
        }
        const int ch0 = (tile == 0 ? 32 * jc : C + 32 * jc) + 4 * hh;       // accumulator rows (r&3) + 8 (r>>2) + 4 hh = channels
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(Wd + 10 * 2 * C + ch0 + 8 * g);
          f32x4 o = {acc[4 * g] + bv[0], acc[4 * g + 1] + bv[1], acc[4 * g + 2] + bv[2], acc[4 * g + 3] + bv[3]};
          if (!tvalid) o = (f32x4){0.f, 0.f, 0.f, 0.f};
          *reinterpret_cast<f32x4*>(Tt + tokw * NF_TS + 32 * tile + 8 * g + 4 * hh) = o;
        }
      }
    }
    __syncthreads();                                             // tile complete; the weight slots are free
    if (jc + 1 < NCH) wload(jc + 1);                             // next chunk's weights travel under the depth-wise phase
    // ---- depth-wise 3x3 on both halves, gate, store, pool partials -------------------------------------------------------------
    {
      const int chA = 32 * jc + 4 * c4, chB = C + chA;
      f32x4 ua[2], psum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int half = 0; half < 2; ++half) {                     // one half's nine tap weights live at a time (36 VGPRs, not 72)
        const int ch = half ? chB : chA;
        f32x4 wt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wt[k] = *reinterpret_cast<const f32x4*>(Wd + k * 2 * C + ch);
        const f32x4 bs = *reinterpret_cast<const f32x4*>(Wd + 9 * 2 * C + ch);
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const int px = (tid >> 3) + 64 * k2, py = px >> 4, pxx = px & 15;
          f32x4 a = bs;
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
              a += *reinterpret_cast<const f32x4*>(Tt + ((py + ky) * NF_HW + pxx + kx) * NF_TS + 32 * half + 4 * c4) * wt[ky * 3 + kx];
          if (half == 0) {
            ua[k2] = a;
          } else {
            const f32x4 g = ua[k2] * a;
            if (y0 + py < p.H && x0 + pxx < p.W) {
              *reinterpret_cast<f32x4*>(p.out + ((long long)(y0 + py) * p.W + x0 + pxx) * p.ldo + chA) = g;
              psum += g;
            }
          }
        }
        asm volatile("" : "+v"(ua[0]), "+v"(ua[1]) : : "memory");
      }
      // lanes with the same channel quad: lane & 7 -> xor 8, 16, 32; then the eight waves through LDS (fixed order: deterministic)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float s = psum[e];
        s += __shfl_xor(s, 8);
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        psum[e] = s;
      }
      if (lane < 8) *reinterpret_cast<f32x4*>(red + (wid * 8 + lane) * 4) = psum;
    }
    if (jc + 1 < NCH) wstore();
    __syncthreads();                                             // tile consumed, next weights in place, wave sums visible
    if (tid < 32) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) s += red[(w * 8 + (tid >> 2)) * 4 + (tid & 3)];
      p.part[(long long)blockIdx.x * C + 32 * jc + tid] = s;
    }
    // (red is rewritten only after the next chunk's first barrier)
  }
}
