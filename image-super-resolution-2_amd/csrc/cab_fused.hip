// HAT's CAB in one launch, plain bf16: conv 180->60 + GELU, conv 60->180, the bf16 store of c2 and the pool partial rows of the
// channel-attention gate (hat_arch.py:121-130 and :50).  The two launches of conv3x3_halo.hip it replaces passed c1 through HBM: conv1's
// store epilogue, conv2's input staging and a launch boundary existed only for that.  Here one workgroup of 8 waves owns one 16x16 output
// tile of one image and keeps its 18x18 c1 tile (the pixels conv2 reads) in LDS:
//   phase 1  conv1 over the 18x18 c1 positions = 324 rows (11 m-tiles of 32, the last 28 rows idle) x 64 channels, K = 3 chunks x 9 taps x 64:
//            the 20x20 input halo of xn is staged one 64-channel chunk at a time (positions outside the image are zero), the weights are
//            cab0's `halo1` image (bn 64, one 9 KB tile per chunk and tap) streaming through a five-slot LDS-DMA ring with counted vmcnt.
//            A lane finds its pixel q at tile row q / 18, column q % 18.  The 22 accumulator tiles go (m = wave / 2 + 4 i, n = wave % 2).
//   phase 2  c1 = bf16(gelu(acc + bias)) into the 18x18x64 LDS tile, in the compact NTERMS == 1 geometry of conv3x3_halo.hip; positions outside
//            the image and channels 60..63 are ZERO (conv2 zero-pads c1, it does not see conv1 of a zero-padded input).
//   phase 3  conv2 over the c1 tile exactly as conv3x3_halo_kernel<4,2,2,3,32,.,2,1>: M = 256, N = 192, K = 9 taps x 2 halves x 32, cab2's
//            `halo1` image (bn 192) through a four-slot ring in the space phase 1 freed.
//   phase 4  conv3x3_halo_vec_epilogue.inc, the text conv3x3_halo_kernel runs.
// Bits: every output element sees the MFMA instruction (32x32x16 bf16), the operand layout and the k-order of the launches replaced (conv1:
// chunk, tap, k-step; conv2: tap, half, k-step), c1 is rounded once at the same point, and the partial row is reduced by the same text and
// indexed by the same block -> tile map (grouped by image).  So c2 and the partial rows are bit for bit those of the two launches.
//   LDS: input chunk 20 x 3104 B | c1 tile 18 x 2816 B | conv1 ring 5 x 9216 B = 158 848 B.  The input rows are 20 pixels x 144 B = 720 dwords
//   padded to 776 == 18 x 36 (mod 64 banks): stepping from pixel q to q + 1 advances 36 dwords across the row wrap too, the conflict-free
//   pattern of the two-rows-of-16 geometry.  conv2's ring (4 x 15 360 B) and the epilogue's patches (45 056 B) reuse the input chunk's space.
#include "ff_common.h"

extern "C" long long ff_conv3x3_halo_weight_bytes(int Cout, int Cin, int bn, int nterms);

struct CabParams {
  const __bf16* in; const unsigned char* w1; const unsigned char* w2; const float* bias1;
  // the names conv3x3_halo_vec_epilogue.inc reads (conv2's side)
  const float* bias; const float* mul; const float* res; float* out; float* pool_part;
  int B, H, W, Cin, ldi, Cmid, Cout, ldo, ldr, tiles_x, tiles_y, io_bf16;
  float alpha;
  FF_STAMP_MEMBER
};

#define CAB_ROWB 144                    // bytes per pixel row (64 bf16 + 16 B pad)
#define CAB_XPROW 3104                  // bytes per input-tile row of 20 pixels
#define CAB_CPROW 2816                  // bytes per c1-tile row of 18 pixels (HaloGeom<1>::PROW)
#define CAB_XBYTES (20 * CAB_XPROW)
#define CAB_CBYTES (18 * CAB_CPROW)
#define CAB_W1SLOT 9216                 // 64 rows x 144 B
#define CAB_W1SLOTS 5
#define CAB_W2SLOT 15360                // 192 rows x 80 B
#define CAB_W2SLOTS 4
#define CAB_LDS (CAB_XBYTES + CAB_CBYTES + CAB_W1SLOTS * CAB_W1SLOT)
static_assert(CAB_LDS <= FF_LDS_MAX, "LDS budget");
static_assert(CAB_W2SLOTS * CAB_W2SLOT <= CAB_XBYTES, "conv2's weight ring lives in the input chunk's space");
static_assert(CAB_XPROW % 16 == 0 && (CAB_XPROW / 4) % 64 == (18 * 36) % 64, "input rows continue the 36-dword pixel step across the row wrap");

// s_waitcnt vmcnt(N); the count is an immediate, so every wait is an instantiation and a count the field cannot hold does not compile
template <int N> __device__ __forceinline__ void cab_wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "counted vmcnt out of range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// f(ff_ic<I>{}) for I = BEGIN .. END - 1: an unrolled loop whose index is a constant expression (the counted waits are templates)
template <int BEGIN, int END, class F> __device__ __forceinline__ void cab_static_for(F&& f) {
  if constexpr (BEGIN < END) {
    f(ff_ic<BEGIN>{});
    cab_static_for<BEGIN + 1, END>(f);
  }
}

__global__ __launch_bounds__(512, 1)
void cab_fused_kernel(CabParams p) {
  // conv2's form, under the names the shared epilogue uses
  constexpr int WM = 4, WN = 2, MI = 2, NI = 3, NTERMS = 1, ACT = ACT_NONE;
  constexpr int NW = WM * WN, NT = NW * 64, BN = WN * NI * 32, TN = NI * 32;
  constexpr bool TWO_PER_CU = false;
  constexpr int VEC_EPI_SPACE = CAB_XBYTES;   // the epilogue's pool row and patches live in the input chunk's space (the .inc asserts that they fit)
  constexpr int ROWB = CAB_ROWB, PROW = CAB_CPROW;
  constexpr int W2ROW = 80, W1ROW = 144;
  constexpr int NPX = 400, PPP = NT / 8, NPASS = (NPX + PPP - 1) / PPP;      // staging: 8 lanes (16 B = 8 channels each) per pixel, 64 pixels per pass
  constexpr int NQ = 324, MI1 = 3;
  constexpr int NT1 = 27, DEPTH1 = CAB_W1SLOTS - 1, NT2 = 18, DEPTH2 = CAB_W2SLOTS - 1, XTAP = 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* Xs = smem;
  unsigned char* Cs = smem + CAB_XBYTES;
  unsigned char* W1s = Cs + CAB_CBYTES;
  unsigned char* W2s = smem;

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hh = lane >> 5;
  const int wr = wid / WN, wc = wid % WN;          // conv2: pixel rows 4 wr .. 4 wr + 3, channels 96 wc ..
  const int wm1 = wid >> 1, wn1 = wid & 1;         // conv1: m-tiles wm1 + 4 i, channels 32 wn1 ..
  const bool third = wm1 < 3;                      // m-tile wm1 + 8 exists (11 m-tiles); the two waves without one run it on clamped rows and drop it:
                                                   // their SIMDs carry 3 + 3 tiles like the others, and the tap loop stays free of branches

  // workgroups bi * bpi .. (bi + 1) * bpi - 1 belong to image bi and are remapped among themselves: the tile map (and so the partial rows)
  // of ff_conv3x3_halo_images, which for one image is ff_conv3x3_halo's
  const int bpi = p.tiles_x * p.tiles_y;
  const int b = (int)blockIdx.x / bpi;
  const int L = ff_xcd_remap((int)blockIdx.x - b * bpi, bpi);
  const int tx = L % p.tiles_x, ty = L / p.tiles_x;
  const int y0 = ty * 16, x0 = tx * 16;
  constexpr int n0 = 0;

  // ---- weight rings.  A wave's pieces per tile differ (9 over 8 waves, 15 over 8 waves): every wave counts its own -----------------------
  auto dma1 = [&](int T, int slot) {
    const unsigned char* src = p.w1 + (long long)T * CAB_W1SLOT + lane * 16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pc = wid + NW * i;
      if (pc < 9)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + pc * 1024),
                                         (__attribute__((address_space(3))) void*)(W1s + slot * CAB_W1SLOT + pc * 1024), 16, 0, 0);
    }
  };
  auto dma2 = [&](int T, int slot) {
    const unsigned char* src = p.w2 + (long long)T * CAB_W2SLOT + lane * 16;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pc = wid + NW * i;
      if (pc < 15)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + pc * 1024),
                                         (__attribute__((address_space(3))) void*)(W2s + slot * CAB_W2SLOT + pc * 1024), 16, 0, 0);
    }
  };
  FF_STAMP(8, 0);
#pragma unroll
  for (int d = 0; d < DEPTH1; ++d) dma1(d, d);

  // ---- input halo staging: tile pixel (r, c) is image pixel (y0 - 2 + r, x0 - 2 + c) ---------------------------------------------------------
  const int cg = (tid & 7) * 8, prow = tid >> 3;
  int goff[NPASS];
#pragma unroll
  for (int j = 0; j < NPASS; ++j) {
    const int hp = j * PPP + prow;
    const int hy = hp / 20, hx = hp - hy * 20;
    const int iy = y0 - 2 + hy, ix = x0 - 2 + hx;
    const bool ok = hp < NPX && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
    goff[j] = ok ? ((b * p.H + iy) * p.W + ix) * p.ldi + cg : -1;
  }
  bf16x8 xr[NPASS];
  auto load_x = [&](int chunk) {                   // always NPASS loads per lane (the counted waits below rely on it): the address is clamped, not the load
    const int c0 = chunk * 64;
    const bool cok = c0 + cg < p.Cin;
#pragma unroll
    for (int j = 0; j < NPASS; ++j) {
      const bool ok = cok && goff[j] >= 0;
      xr[j] = *reinterpret_cast<const bf16x8*>(p.in + (ok ? goff[j] + c0 : 0));       // (masked in store_x: nothing here waits for the load)
    }
  };
  auto store_x = [&](int chunk) {
    const int c0 = chunk * 64;
#pragma unroll
    for (int j = 0; j < NPASS; ++j) {
      const int hp = j * PPP + prow;
      const bool ok = goff[j] >= 0;
      bf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (ok && c0 + cg + e < p.Cin) ? xr[j][e] : (__bf16)0.f;   // columns Cin.. of a row are not the tensor's
      if (hp < NPX) *reinterpret_cast<bf16x8*>(Xs + (hp / 20) * CAB_XPROW + (hp % 20) * ROWB + (tid & 7) * 16) = v;
    }
  };
  load_x(0);
  store_x(0);
  FF_STAMP(8, 1);

  // ---- phase 1: conv1 ------------------------------------------------------------------------------------------------------------------
  f32x16 acc1[MI1];
#pragma unroll
  for (int i = 0; i < MI1; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[i][r] = 0.f;
  int aoff1[MI1];
#pragma unroll
  for (int i = 0; i < MI1; ++i) {
    int q = (wm1 + 4 * i) * 32 + l31;
    q = q < NQ ? q : NQ - 1;                        // rows 324.. are computed on a valid address and dropped
    aoff1[i] = (q / 18) * CAB_XPROW + (q % 18) * ROWB + 16 * hh;
  }
  const int boff1 = (wn1 * 32 + l31) * W1ROW + 16 * hh;

  cab_static_for<0, NT1>([&](auto Tc) {
    constexpr int T = decltype(Tc)::value, chunk = T / 9, tap = T - 9 * chunk;
    constexpr bool more_x = chunk + 1 < 3;
    constexpr int dy = tap / 3, dx = tap - 3 * dy;
    // Tile T's pieces of this wave have landed: younger than them are the tiles T + 1 .. T + DEPTH1 - 1 and, at the taps after XTAP, the
    // NPASS input loads of the next chunk (issued after tap XTAP's DMA; vmcnt retires in issue order).  Wave 0 issues two pieces per tile,
    // the others one.  Then the wave's own LDS traffic is done, and the raw barrier (no vmcnt(0) drain) publishes the tile and frees the
    // slot of tile T - 1.
    constexpr int young = NT1 - 1 - T < DEPTH1 - 1 ? NT1 - 1 - T : DEPTH1 - 1;
    constexpr int xl = (tap > XTAP && more_x) ? NPASS : 0;
    if (wid == 0) cab_wait_vmcnt<young * 2 + xl>();
    else cab_wait_vmcnt<young + xl>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (T + DEPTH1 < NT1) dma1(T + DEPTH1, (T + DEPTH1) % CAB_W1SLOTS);
    if (tap == XTAP && more_x) {
      asm volatile("" ::: "memory");                // the input loads stay behind this tap's DMA
      load_x(chunk + 1);
      asm volatile("" ::: "memory");
    }
    const unsigned char* xa = Xs + dy * CAB_XPROW + dx * ROWB;
    const unsigned char* wb = W1s + (T % CAB_W1SLOTS) * CAB_W1SLOT;
    bf16x8 ah[4][MI1], bh[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int i = 0; i < MI1; ++i) ah[s][i] = *reinterpret_cast<const bf16x8*>(xa + aoff1[i] + 32 * s);
      bh[s] = *reinterpret_cast<const bf16x8*>(wb + boff1 + 32 * s);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc1[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s][0], bh[s], acc1[0], 0, 0, 0);
      acc1[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s][1], bh[s], acc1[1], 0, 0, 0);
      acc1[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s][2], bh[s], acc1[2], 0, 0, 0);
    }
    if (tap == 8 && more_x) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                 // every wave is done reading this chunk's input tile
      store_x(chunk + 1);                           // (made visible by the barrier at the top of the next tap)
    }
  });
  FF_STAMP(8, 2);

  // ---- phase 2: the c1 tile.  conv2's first weight tiles land meanwhile, in the input chunk's space ------------------------------------------
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                     // every wave has left conv1's taps (and every conv1 weight tile has landed: the last wait was vmcnt(0))
#pragma unroll
  for (int d = 0; d < DEPTH2; ++d) dma2(d, d);
  {
    const int n = wn1 * 32 + l31;
    const bool nok = n < p.Cmid;
    const float bv = nok ? p.bias1[n] : 0.f;
#pragma unroll
    for (int i = 0; i < MI1; ++i) {
      if (i == 2 && !third) continue;
      const int q0 = (wm1 + 4 * i) * 32 + 4 * hh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {               // register r = tile row (r & 3) + 8 (r >> 2) + 4 hh of channel l31
        const int q = q0 + (r & 3) + 8 * (r >> 2);
        const int cy = q / 18, cx = q - cy * 18;
        const int iy = y0 - 1 + cy, ix = x0 - 1 + cx;
        const bool in_img = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        // the value conv1's epilogue stores: act(acc + bias), then its fma with scale 1 and no residual, rounded to bf16 once
        const float a = __builtin_fmaf(ff_act_c<ACT_GELU, true>(acc1[i][r] + bv), 1.0f, 0.f);
        const __bf16 h = (nok && in_img) ? (__bf16)a : (__bf16)0.f;
        if (q < NQ) *reinterpret_cast<__bf16*>(Cs + cy * PROW + cx * ROWB + n * 2) = h;
      }
    }
  }
  FF_STAMP(8, 3);

  // ---- phase 3: conv2, the tap loop of conv3x3_halo_kernel<4,2,2,3,32,.,.,1> on the c1 tile -------------------------------------------------------
#include "gemm_acc_zero.inc"
  int aoff[MI], boff[NI];
#pragma unroll
  for (int i = 0; i < MI; ++i) aoff[i] = ((wr * MI + i) * 2 + (l31 >> 4)) * PROW + (l31 & 15) * ROWB + 16 * hh;
#pragma unroll
  for (int j = 0; j < NI; ++j) boff[j] = (wc * TN + j * 32 + l31) * W2ROW + 16 * hh;
  // Ring of four slots, three tiles in flight, as in phase 1 (waves 0..6 issue two pieces per tile, wave 7 one).
  cab_static_for<0, NT2>([&](auto Tc) {
    constexpr int T = decltype(Tc)::value, tap = T / 2, half = T & 1;
    constexpr int dy = tap / 3, dx = tap - 3 * dy;
    constexpr int young = NT2 - 1 - T < DEPTH2 - 1 ? NT2 - 1 - T : DEPTH2 - 1;
    if (wid < 7) cab_wait_vmcnt<young * 2>();
    else cab_wait_vmcnt<young>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // (first tile: the wave's c1 writes)
    __builtin_amdgcn_s_barrier();
    if (T + DEPTH2 < NT2) dma2(T + DEPTH2, (T + DEPTH2) % CAB_W2SLOTS);
    const unsigned char* xa = Cs + dy * PROW + dx * ROWB;
    const unsigned char* wb = W2s + (T % CAB_W2SLOTS) * CAB_W2SLOT;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 ah[MI], bh[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) ah[i] = *reinterpret_cast<const bf16x8*>(xa + aoff[i] + 32 * (half * 2 + s));
#pragma unroll
      for (int j = 0; j < NI; ++j) bh[j] = *reinterpret_cast<const bf16x8*>(wb + boff[j] + 32 * s);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
    }
  });
  FF_STAMP(8, 4);
  // ---- phase 4: conv2's vector epilogue (bias, bf16 rows of c2, the workgroup's pool partial row) ---------------------------------------------
  {
#include "conv3x3_halo_vec_epilogue.inc"
  }
  FF_STAMP(8, 5);
  FF_STAMP_DRAINED(8, 6);
}

// CAB on bf16 rows: c2 = conv3x3(gelu(conv3x3(xn) + b1)) + b2 and, per workgroup, the channel sums of c2 (fp32, before rounding).
extern "C" int ff_cab_fused(const void* xn, int ldi, const void* w1_img, long long w1_bytes, const float* bias1,
                            const void* w2_img, long long w2_bytes, const float* bias2, void* c2, int ldo, float* pool_partials,
                            int B, int H, int W, int Cin, int Cmid, int Cout, int nterms, int io_bf16, void* stream) {
  FF_CHECK_ARG(nterms == 1, "ff_cab_fused: plain bf16 only (nterms must be 1)");
  FF_CHECK_ARG(io_bf16 == 3, "ff_cab_fused: xn and c2 must be bf16 rows (io_bf16 == 3)");
  FF_CHECK_ARG(Cin == 180 && Cmid == 60 && Cout == 180, "ff_cab_fused: built for 180 -> 60 -> 180 channels");
  FF_CHECK_ARG(B > 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "ff_cab_fused: H and W must be multiples of 16");
  FF_CHECK_ARG((long long)H * W >= 1024, "ff_cab_fused: H * W must be at least 1024");
  FF_CHECK_ARG(xn && w1_img && w2_img && bias1 && bias2 && c2 && pool_partials, "ff_cab_fused: null pointer");
  FF_CHECK_ARG(ldi % 8 == 0 && ldi >= Cin && (((uintptr_t)xn) & 15) == 0, "ff_cab_fused: xn rows must be 16-byte aligned (pitch %% 8 == 0)");
  FF_CHECK_ARG(ldo % 4 == 0 && ldo >= Cout && (((uintptr_t)c2) & 15) == 0, "ff_cab_fused: c2 rows must be 8-byte aligned (pitch %% 4 == 0) on a 16-byte aligned base");
  FF_CHECK_ARG((((uintptr_t)w1_img) & 15) == 0 && (((uintptr_t)w2_img) & 15) == 0, "ff_cab_fused: weight images must be 16-byte aligned");
  FF_CHECK_ARG(w1_bytes == ff_conv3x3_halo_weight_bytes(Cmid, Cin, 64, 1), "ff_cab_fused: conv1's weight image is not the bn 64 halo image of its shape");
  FF_CHECK_ARG(w2_bytes == ff_conv3x3_halo_weight_bytes(Cout, Cmid, 192, 1), "ff_cab_fused: conv2's weight image is not the bn 192 halo image of its shape");
  FF_CHECK_ARG((long long)B * H * W * ldi < (1LL << 31) && (long long)B * H * W * ldo < (1LL << 31), "ff_cab_fused: rows too large for 32-bit offsets (B * H * W * pitch >= 2^31)");
  FF_CHECK_ARG(xn != c2, "ff_cab_fused: c2 must not alias xn");
  CabParams p;
  p.in = (const __bf16*)xn; p.w1 = (const unsigned char*)w1_img; p.w2 = (const unsigned char*)w2_img; p.bias1 = bias1;
  p.bias = bias2; p.mul = nullptr; p.res = nullptr; p.out = (float*)c2; p.pool_part = pool_partials;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.ldi = ldi; p.Cmid = Cmid; p.Cout = Cout; p.ldo = ldo; p.ldr = 0;
  p.tiles_x = W / 16; p.tiles_y = H / 16; p.io_bf16 = io_bf16; p.alpha = 1.0f;
  FF_STAMP_ARM(p);
  static ff_device_once once;
  if (!ff_raise_lds(once, "ff_cab_fused", CAB_LDS, FF_LDS_SAY_SIZE | FF_LDS_SAY_ERR, &cab_fused_kernel)) return FF_ERR_LAUNCH;
  const long long nblocks = (long long)B * p.tiles_x * p.tiles_y;     // (< 2^31 / (256 * 184) by the offset check)
  hipLaunchKernelGGL(cab_fused_kernel, dim3((unsigned)nblocks), dim3(512), CAB_LDS, (hipStream_t)stream, p);
  FF_LAUNCH_CHECK("ff_cab_fused");
  return FF_OK;
}
