// out[M][N] = epilogue(A[M][K] . W[N][K]^T) for bf16 ROWS: NAFNet's deep 1x1 convolutions (c = 256 / 512 / 1024) in plain-bf16 mode,
// where LayerNorm and the SimpleGate epilogue already store the activation as the bf16 the MFMA would round it to.
//
// Same arithmetic as conv_igemm_bf16_kernel<.., NTERMS = 1> (conv_gemm_bf16.hip), so the results are bit-equal to it: one
// v_mfma_f32_32x32x16_bf16 per 16 k-values into the same fp32 accumulator, k ascending, and the same epilogue expressions.
// What differs is how the operands reach LDS:
//   - A is bf16 [M][lda] and W the hi plane of ff_split_bf16 [N][K]; both go global -> LDS by LDS-DMA (global_load_lds_dwordx4):
//     no VGPR staging, no conversion, no staging stores, half the A bytes;
//   - BK = 64, two LDS buffers, ONE barrier per chunk: the barrier at the top of step c says "chunk c landed" (every wave waited
//     for its own DMA pieces) and "everybody is done reading the other buffer", so the DMA of chunk c + 1 is issued right behind
//     it and stays in flight under the 16 k-steps of chunk c;
//   - the LDS image of a tile is [row][64 bf16] = 128-byte rows, lane-linear per DMA piece (8 rows x 128 B = 1 KiB per wave
//     instruction).  A ds_read_b128 lane group is 16 rows at one 16-byte slot; on linear 128-byte rows those share two slots of the
//     256-byte bank row (8-way).  The slot is therefore XORed with (row >> 1) & 7 -- on the per-lane SOURCE address of the DMA and
//     on the read address (guide section 5.4 rule 21) -- which puts the 16 rows of every lane group on 16 distinct slots.
// A32 (conv3, whose A operand is scaled per input channel in fp32 before it is rounded -- kmul -- and so has to stay fp32 in memory):
// the same loop with the A tile staged through registers, one chunk ahead: loaded right behind the barrier, multiplied, rounded and
// written to the (equally swizzled) LDS image at the top of the next step; W still arrives by LDS-DMA.
// Tiles: 128 x 128 and 128 x 64, eight waves (64 x 32 / 32 x 32 per wave, two waves per SIMD and workgroup).
#include "ff_common.h"

struct RowsGemmParams {
  const void* a;      // bf16 [M][lda], or fp32 [M][lda] (A32)
  const float* kmul;  // A32 only, optional [K]: A is scaled per input channel in fp32 before the bf16 rounding
  const __bf16* w;
  const float* bias;
  const float* mul;
  const float* res;
  void* out;          // GATE: bf16 [M][ldo] (N / 2 channels); else fp32 [M][ldo]
  int M, N, K;
  int lda, ldo, ldr;
  int rpi;            // KMI form: rows per image; kmul is [M / rpi][K] and row m is scaled by kmul[m / rpi]
};

// KMI (A32 only): kmul is looked up per STAGED ROW -- each of a thread's AS rows carries its own image's scale vector, so an m-tile may
// hold rows of several images and the tiling (and every other line of the kernel) stays the single-image one.  A row's dot product does
// not depend on which tile holds it, so the rows are bit-equal to the single-image launch on their image alone.
template <int BM, int BN, int WM, int WN, bool GATE, bool A32, bool KMI>
__device__ __forceinline__ void gemm_rows_bf16_body(const RowsGemmParams& p) {
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int MI = TM / 32, NI = TN / 32;
  constexpr int AI = A32 ? 0 : BM / 8 / NW, BI = BN / 8 / NW;    // 1-KiB DMA pieces (8 rows x 128 B) per wave and chunk
  constexpr int AS = A32 ? BM / (8 * NW) : 0;                    // A32: 16-byte LDS slots (8 k-values, 32 B of fp32) per thread and chunk
  constexpr int ABYTES = BM * RG_ROWB, BUFB = gemm_bufb(BM, BN, RG_ROWB);     // the map [2][A tile | B tile]: lds_layout.h
  static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "DMA pieces must tile the waves");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2][A tile | B tile]; the epilogue patch reuses it

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int wr = wid / WN, wc = wid % WN;

  const int mtiles = (p.M + BM - 1) / BM, ntiles = (p.N + BN - 1) / BN;
  const int L = ff_xcd_remap(blockIdx.x, mtiles * ntiles);
  const int m0 = (L / ntiles) * BM, n0 = (L % ntiles) * BN;

  // DMA sources: lane l of piece pc fills LDS row 8 pc + (l >> 3), physical slot l & 7, with the row's logical slot
  // (l & 7) ^ ((row >> 1) & 7).  Rows beyond M / N are clamped to the last one: read in bounds, never stored.
  const __bf16* asrc[AI + 1];
  const __bf16* bsrc[BI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    const int row = 8 * (wid + NW * i) + (lane >> 3);
    const int q = (lane & 7) ^ ((row >> 1) & 7);
    const int m = m0 + row < p.M ? m0 + row : p.M - 1;
    asrc[i] = reinterpret_cast<const __bf16*>(p.a) + (long long)m * p.lda + 8 * q;
  }
  // A32: thread t stages logical slot t & 7 of rows (t >> 3) + 8 NW i -- eight lanes read 256 contiguous bytes of a row
  const float* fsrc[AS + 1];
  int fdst[AS + 1];
  f32x4 ra[AS + 1][2], km[2];
  const float* ksrc[KMI ? AS + 1 : 1];
  f32x4 kmi[KMI ? AS + 1 : 1][2];
#pragma unroll
  for (int i = 0; i < AS; ++i) {
    const int row = (tid >> 3) + 8 * NW * i, q = tid & 7;
    const int m = m0 + row < p.M ? m0 + row : p.M - 1;
    fsrc[i] = reinterpret_cast<const float*>(p.a) + (long long)m * p.lda + 8 * q;
    fdst[i] = row * 128 + (q ^ ((row >> 1) & 7)) * 16;
    if constexpr (KMI) ksrc[i] = p.kmul + (long long)(m / p.rpi) * p.K + 8 * q;      // (m is clamped into [0, M): a valid image)
  }
  auto load_a = [&](int c) {
#pragma unroll
    for (int i = 0; i < AS; ++i) {
      ra[i][0] = *reinterpret_cast<const f32x4*>(fsrc[i] + 64 * c);
      ra[i][1] = *reinterpret_cast<const f32x4*>(fsrc[i] + 64 * c + 4);
    }
    if constexpr (KMI) {
#pragma unroll
      for (int i = 0; i < AS; ++i) {
        kmi[i][0] = *reinterpret_cast<const f32x4*>(ksrc[i] + 64 * c);
        kmi[i][1] = *reinterpret_cast<const f32x4*>(ksrc[i] + 64 * c + 4);
      }
    } else if (p.kmul) {
      km[0] = *reinterpret_cast<const f32x4*>(p.kmul + 64 * c + 8 * (tid & 7));
      km[1] = *reinterpret_cast<const f32x4*>(p.kmul + 64 * c + 8 * (tid & 7) + 4);
    }
  };
  auto store_a = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AS; ++i) {
      f32x4 u = ra[i][0], v = ra[i][1];
      if constexpr (KMI) { u *= kmi[i][0]; v *= kmi[i][1]; }
      else if (p.kmul) { u *= km[0]; v *= km[1]; }
      const bf16x8 h = {(__bf16)u[0], (__bf16)u[1], (__bf16)u[2], (__bf16)u[3], (__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
      *reinterpret_cast<bf16x8*>(smem + buf * BUFB + fdst[i]) = h;
    }
  };
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int row = 8 * (wid + NW * i) + (lane >> 3);
    const int q = (lane & 7) ^ ((row >> 1) & 7);
    const int n = n0 + row < p.N ? n0 + row : p.N - 1;
    bsrc[i] = p.w + (long long)n * p.K + 8 * q;
  }
  auto dma = [&](int c, int buf) {
    unsigned char* dst = smem + buf * BUFB;
#pragma unroll
    for (int i = 0; i < AI; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + 64 * c),
                                       (__attribute__((address_space(3))) void*)(dst + (wid + NW * i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < BI; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc[i] + 64 * c),
                                       (__attribute__((address_space(3))) void*)(dst + ABYTES + (wid + NW * i) * 1024), 16, 0, 0);
  };

#include "gemm_acc_zero.inc"

  const int sw = (l31 >> 1) & 7;                    // tile rows are multiples of 32 apart: the swizzle depends on l31 only
  const int arow = (wr * TM + l31) * 128, brow = ABYTES + (wc * TN + l31) * 128;
  const int nchunks = p.K / 64;
  if (A32) load_a(0);
  dma(0, 0);
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (A32) store_a(buf);                             // chunk c's A, loaded a step ago; buffer buf was last read in step c - 2
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of chunk c landed
    __syncthreads();                                   // ... everybody's did, and nobody still reads buffer buf ^ 1
    if (c + 1 < nchunks) {
      if (A32) load_a(c + 1);
      dma(c + 1, buf ^ 1);
    }
    const unsigned char* base = smem + buf * BUFB;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int slot = ((2 * s + hh) ^ sw) * 16;
      bf16x8 a[MI], b[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) a[i] = *reinterpret_cast<const bf16x8*>(base + arow + i * 32 * 128 + slot);
#pragma unroll
      for (int j = 0; j < NI; ++j) b[j] = *reinterpret_cast<const bf16x8*>(base + brow + j * 32 * 128 + slot);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  __syncthreads();                                     // the staging buffers become the epilogue's wave-private patches

  // Epilogues: the expressions of conv_igemm_bf16_kernel's gate and 16-byte forms, operation for operation.  Each 32(m) x 32(n)
  // accumulator tile is transposed through a wave-private LDS patch so a lane owns consecutive channels of one row.
  float* tr = reinterpret_cast<float*>(smem) + wid * (32 * 36);
  static_assert(gemm_patches_fit(BM, BN, RG_ROWB, NW), "the epilogues' 32 x 36 patches must fit in the idle staging buffers");
  if (GATE) {
    // SimpleGate on interleaved columns: out[m][j] = y[m][2j] * y[m][2j+1], rounded to the bf16 its only consumer (conv5's A
    // operand) would round it to
    __bf16* out = reinterpret_cast<__bf16*>(p.out);
    const int grow = lane >> 2, seg = lane & 3;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = n0 + wc * TN + j * 32 + l31;
      const float bv = (p.bias && n < p.N) ? p.bias[n] : 0.f;
      const int nq = (n0 + wc * TN + j * 32) / 2 + 4 * seg;      // first of this lane's four output channels
      const bool nqok = nq < p.N / 2;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int mb = m0 + wr * TM + i * 32;
#pragma unroll
        for (int r = 0; r < 16; ++r) tr[((r & 3) + 8 * (r >> 2) + 4 * hh) * 36 + l31] = acc[i][j][r] + bv;
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          const int row = grow + 16 * pass;
          const f32x4 a = *reinterpret_cast<const f32x4*>(tr + row * 36 + 8 * seg);
          const f32x4 b2 = *reinterpret_cast<const f32x4*>(tr + row * 36 + 8 * seg + 4);
          const f32x4 o = {a[0] * a[1], a[2] * a[3], b2[0] * b2[1], b2[2] * b2[3]};
          const bf16x4 ob = {(__bf16)o[0], (__bf16)o[1], (__bf16)o[2], (__bf16)o[3]};
          const int m = mb + row;
          if (nqok && m < p.M) *reinterpret_cast<bf16x4*>(out + (long long)m * p.ldo + nq) = ob;
        }
      }
    }
  } else {
    float* out = reinterpret_cast<float*>(p.out);
    const bool has_res = p.res != nullptr;
    const int tq = lane >> 3, q4 = 4 * (lane & 7);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = n0 + wc * TN + j * 32 + l31;
      const int nc = n < p.N ? n : 0;
      const float bv = p.bias ? p.bias[nc] : 0.f;
      const float mv = p.mul ? p.mul[nc] : 1.f;
      const int nq = n0 + wc * TN + j * 32 + q4;
      const bool nqok = nq < p.N;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int mb = m0 + wr * TM + i * 32;
        f32x4 rq[4];
        long long oo[4];
        bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int m = mb + tq + 8 * k;
          ok[k] = nqok && m < p.M;
          oo[k] = ok[k] ? (long long)m * p.ldo + nq : 0;
          f32x4 r0 = {0.f, 0.f, 0.f, 0.f};
          if (has_res) { const f32x4 u = *reinterpret_cast<const f32x4*>(p.res + (ok[k] ? (long long)m * p.ldr + nq : 0)); r0 = ok[k] ? u : r0; }
          rq[k] = r0;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) tr[((r & 3) + 8 * (r >> 2) + 4 * hh) * 36 + l31] = (acc[i][j][r] + bv) * mv;
        f32x4 ov[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) ov[k] = *reinterpret_cast<const f32x4*>(tr + (tq + 8 * k) * 36 + q4) + rq[k];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (ok[k]) *reinterpret_cast<f32x4*>(out + oo[k]) = ov[k];
      }
    }
  }
}

template <int BM, int BN, int WM, int WN, bool GATE, bool A32>
__global__ __launch_bounds__(WM * WN * 64) void gemm_rows_bf16_kernel(RowsGemmParams p) {
  gemm_rows_bf16_body<BM, BN, WM, WN, GATE, A32, false>(p);
}

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void gemm_rows_bf16_kmimg_kernel(RowsGemmParams p) {
  gemm_rows_bf16_body<BM, BN, WM, WN, false, true, true>(p);
}

template <int BM, int BN, int WM, int WN>
static int launch_rows_kmimg(const RowsGemmParams& p, hipStream_t st) {
  constexpr size_t lds = gemm_lds(BM, BN, RG_ROWB);
  static_assert(lds <= FF_LDS_DEFAULT_MAX, "LDS budget");
  dim3 grid((unsigned)(ff_cdiv(p.M, BM) * ff_cdiv(p.N, BN))), block(WM * WN * 64);
  hipLaunchKernelGGL((gemm_rows_bf16_kmimg_kernel<BM, BN, WM, WN>), grid, block, lds, st, p);
  FF_LAUNCH_CHECK("ff_gemm_rows_bf16_kmul_images");
  return FF_OK;
}

template <int BM, int BN, int WM, int WN>
static int launch_rows(const RowsGemmParams& p, bool gate, bool a32, hipStream_t st) {
  constexpr size_t lds = gemm_lds(BM, BN, RG_ROWB);
  static_assert(lds <= FF_LDS_DEFAULT_MAX, "LDS budget (two staging buffers; the epilogue patches reuse them: asserted in the kernel)");
  dim3 grid((unsigned)(ff_cdiv(p.M, BM) * ff_cdiv(p.N, BN))), block(WM * WN * 64);
  if (a32)                                                 // conv3: residual epilogue only
    hipLaunchKernelGGL((gemm_rows_bf16_kernel<BM, BN, WM, WN, false, true>), grid, block, lds, st, p);
  else if (gate)
    hipLaunchKernelGGL((gemm_rows_bf16_kernel<BM, BN, WM, WN, true, false>), grid, block, lds, st, p);
  else
    hipLaunchKernelGGL((gemm_rows_bf16_kernel<BM, BN, WM, WN, false, false>), grid, block, lds, st, p);
  FF_LAUNCH_CHECK("ff_gemm_rows_bf16");
  return FF_OK;
}

// The tile configuration ff_gemm_rows_bf16 picks for tile_hint <= 0 (the table in ff_gemm_rows_bf16).  Exported so that a caller that batches
// independent images can pass the configuration ONE image's row count would get as its tile_hint.
extern "C" int ff_gemm_rows_bf16_tile(long long M, int N) {
  return (long long)ff_cdiv(M, 128) * ff_cdiv(N, 128) <= 256 ? 2 : 1;
}

extern "C" int ff_gemm_rows_bf16(const void* a, int a_fp32, int lda, const void* w_hi, int Kp, const float* kmul, const float* bias,
                                 const float* mul, const float* res, int ldr, void* out, int ldo, long long M, int N, int K, int gate,
                                 int tile_hint, void* stream) {
  FF_CHECK_ARG(a && w_hi && out, "ff_gemm_rows_bf16: null pointer");
  FF_CHECK_ARG(M > 0 && M < (1LL << 31) && N > 0 && K > 0, "ff_gemm_rows_bf16: bad dims");
  FF_CHECK_ARG(K % 64 == 0 && Kp == K, "ff_gemm_rows_bf16: needs K %% 64 == 0 and an unpadded weight plane (Kp == K), got K=%d Kp=%d", K, Kp);
  FF_CHECK_ARG(a_fp32 == 0 || a_fp32 == 1, "ff_gemm_rows_bf16: a_fp32 must be 0 or 1");
  FF_CHECK_ARG(lda >= K && lda % (a_fp32 ? 4 : 8) == 0 && (((uintptr_t)a) & 15) == 0 && (((uintptr_t)w_hi) & 15) == 0,
               "ff_gemm_rows_bf16: A rows and the weight plane must be 16-byte aligned (lda %% 8 == 0, fp32 rows lda %% 4 == 0; lda >= K)");
  FF_CHECK_ARG(gate == 0 || gate == 1, "ff_gemm_rows_bf16: gate must be 0 or 1");
  FF_CHECK_ARG(!a_fp32 || !gate, "ff_gemm_rows_bf16: fp32 A rows come with the fp32-rows epilogue only");
  FF_CHECK_ARG(!kmul || (a_fp32 && (((uintptr_t)kmul) & 15) == 0), "ff_gemm_rows_bf16: kmul scales fp32 A rows only and must be 16-byte aligned");
  if (gate) {
    FF_CHECK_ARG(N % 8 == 0 && !res && !mul && ldo >= N / 2 && ldo % 4 == 0 && (((uintptr_t)out) & 7) == 0,
                 "ff_gemm_rows_bf16: the pair-product epilogue needs N %% 8 == 0, no residual / scale and 8-byte aligned bf16 output rows");
  } else {
    FF_CHECK_ARG(N % 4 == 0 && ldo >= N && ldo % 4 == 0 && (((uintptr_t)out) & 15) == 0,
                 "ff_gemm_rows_bf16: needs N %% 4 == 0 and 16-byte aligned output rows");
    FF_CHECK_ARG(!res || (ldr >= N && ldr % 4 == 0 && (((uintptr_t)res) & 15) == 0), "ff_gemm_rows_bf16: residual rows must be 16-byte aligned");
  }
  RowsGemmParams p;
  p.a = a; p.kmul = kmul; p.w = (const __bf16*)w_hi; p.bias = bias; p.mul = mul; p.res = res; p.out = out;
  p.M = (int)M; p.N = N; p.K = K; p.lda = lda; p.ldo = ldo; p.ldr = ldr; p.rpi = 0;
  hipStream_t st = (hipStream_t)stream;
  int cfg = tile_hint;
  // Measured on MI355X, one process, variants alternating, median us per launch (profiles/nafnet_rows_gemm.json; old = ff_conv2d_bf16s
  // on fp32 rows; "scaled" = fp32 A rows with kmul).  Four-wave forms of both tiles (64 x 64 / 64 x 32 per wave) were measured too and
  // won nowhere by more than their spread: they are not kept.
  //   M x K -> N, epilogue                 old   128x128  128x64
  //   4096 x 1024 -> 2048 bias             47.9    27.3    32.7
  //   4096 x 1024 -> 1024 scaled residual  42.8    23.6    24.5     (256 tiles: the two forms tie within their spread)
  //   4096 x 1024 -> 2048 gate             39.8    21.2    27.4
  //   4096 x 1024 -> 1024 residual         35.4    17.9    16.9     <- 256 tiles of 128 x 128 = one per CU: the narrow tile gives two
  //   16384 x 512 -> 1024 bias             47.4    26.4    28.6
  //   16384 x 512 ->  512 scaled residual  32.1    22.1    27.6
  //   16384 x 512 -> 1024 gate             42.1    22.4    25.5
  //   16384 x 512 ->  512 residual         28.2    18.7    21.0
  //   65536 x 256 ->  512 bias             56.4    33.3    35.6
  //   65536 x 256 ->  256 scaled residual  40.3    31.4    33.8
  //   65536 x 256 ->  512 gate             48.3    26.0    30.1
  //   65536 x 256 ->  256 residual         37.8    27.0    29.2
  // Every shape is faster than the old route by more than the spread of its repeats, so none stays behind.
  if (cfg <= 0) cfg = ff_gemm_rows_bf16_tile(M, N);
  switch (cfg) {
    case 1: return launch_rows<128, 128, 2, 4>(p, gate != 0, a_fp32 != 0, st);      // 64 x 32 per wave
    case 2: return launch_rows<128, 64, 4, 2>(p, gate != 0, a_fp32 != 0, st);       // 32 x 32 per wave
    default: ff_set_error("ff_gemm_rows_bf16: bad tile_hint %d", cfg); return FF_ERR_ARG;
  }
}

// conv3 of B independent images in one launch: a is fp32 [M][lda], M == B * rows_per_image, and kmul is [B][K] -- row m is scaled by
// kmul[m / rows_per_image] before the bf16 rounding.  The fp32-rows epilogue (bias, * mul, + res).  Every row is bit-equal to
// ff_gemm_rows_bf16(a_fp32 = 1, kmul = kmul[b]) on its image alone; tile_hint <= 0 takes the configuration of ONE image's rows.
extern "C" int ff_gemm_rows_bf16_kmul_images(const float* a, int lda, const void* w_hi, int Kp, const float* kmul, int B, int rows_per_image,
                                             const float* bias, const float* mul, const float* res, int ldr, float* out, int ldo,
                                             long long M, int N, int K, int tile_hint, void* stream) {
  FF_CHECK_ARG(a && w_hi && kmul && out, "ff_gemm_rows_bf16_kmul_images: null pointer");
  FF_CHECK_ARG(B >= 1 && rows_per_image >= 1 && M == (long long)B * rows_per_image && M < (1LL << 31),
               "ff_gemm_rows_bf16_kmul_images: M must be B * rows_per_image and below 2^31 (got M=%lld B=%d rows_per_image=%d)", M, B, rows_per_image);
  FF_CHECK_ARG(N > 0 && K > 0 && K % 64 == 0 && Kp == K, "ff_gemm_rows_bf16_kmul_images: needs K %% 64 == 0 and an unpadded weight plane (Kp == K), got K=%d Kp=%d", K, Kp);
  FF_CHECK_ARG(lda >= K && lda % 4 == 0 && (((uintptr_t)a) & 15) == 0 && (((uintptr_t)w_hi) & 15) == 0 && (((uintptr_t)kmul) & 15) == 0,
               "ff_gemm_rows_bf16_kmul_images: A rows, the weight plane and kmul must be 16-byte aligned (lda %% 4 == 0, lda >= K)");
  FF_CHECK_ARG(N % 4 == 0 && ldo >= N && ldo % 4 == 0 && (((uintptr_t)out) & 15) == 0,
               "ff_gemm_rows_bf16_kmul_images: needs N %% 4 == 0 and 16-byte aligned output rows");
  FF_CHECK_ARG(!res || (ldr >= N && ldr % 4 == 0 && (((uintptr_t)res) & 15) == 0), "ff_gemm_rows_bf16_kmul_images: residual rows must be 16-byte aligned");
  RowsGemmParams p;
  p.a = a; p.kmul = kmul; p.w = (const __bf16*)w_hi; p.bias = bias; p.mul = mul; p.res = res; p.out = out;
  p.M = (int)M; p.N = N; p.K = K; p.lda = lda; p.ldo = ldo; p.ldr = ldr; p.rpi = rows_per_image;
  hipStream_t st = (hipStream_t)stream;
  int cfg = tile_hint;
  if (cfg <= 0) cfg = ff_gemm_rows_bf16_tile(rows_per_image, N);
  switch (cfg) {
    case 1: return launch_rows_kmimg<128, 128, 2, 4>(p, st);
    case 2: return launch_rows_kmimg<128, 64, 4, 2>(p, st);
    default: ff_set_error("ff_gemm_rows_bf16_kmul_images: bad tile_hint %d", cfg); return FF_ERR_ARG;
  }
}
