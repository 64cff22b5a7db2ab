// The implicit-GEMM kernel (conv_gemm_bf16.hip includes this file twice).  CIG_KERNEL names the kernel; CIG_KMUL_IMAGES = 0 is the kernel of
// ff_conv2d_bf16s.  CIG_KMUL_IMAGES = 1 (1x1, VEC4): kmul is [B][Cin] and A row m is scaled by its image's vector, kmul[a_b][ci] -- conv3 of
// B independent images in one launch (ff_conv2d_bf16s_kmul_images calls it with B = B, H = 1, W = rows per image, so a_b IS the image).
// CIG_W_IMAGES = 1 (1x1, VEC4): the weight planes are [B][Cout][Kp] and an m-tile multiplies by the planes of the image its first row
// belongs to (ff_conv2d_bf16s_wimages: H = 1, W = rows per image, a multiple of the tile height, so a tile never straddles two images) --
// DAT's att = v . wbd^T with one block-diagonal matrix per image.  Nothing else differs.
// BKB = k-values per chunk (one barrier per chunk).  32: the original form.  64 (r2): twice the MFMAs between barriers -- the
// 8-wave 128-row tiles issue only 12 MFMAs per wave and chunk at 32, and the barrier + staging round trip per chunk, not the
// MFMA pipe, set their time (SQ counters, tools/gemm_prof.py: MFMA pipe 28 % busy on the 1024 -> 2048 NAFNet GEMM).
//   LDS row = [BKB hi | BKB lo | 16 B pad]: 144 B (36 dwords) or 272 B (68 dwords), both = 4 (mod 32) dwords: conflict-free b128 reads.
template <int BM, int BN, int WM, int WN, bool VEC4, int NTERMS, int BKB>
__global__ __launch_bounds__(WM * WN * 64) void CIG_KERNEL(ConvBfParams p) {
  constexpr int ROWB = cig_rowb(BKB), PLB = BKB * 2;  // bytes per LDS row / per plane of a row (the map: lds_layout.h)
  constexpr int KQ = BKB / 4, QB = BKB / 8;       // 4-float quads / 16-byte bf16 items per row and plane
  constexpr int NT = WM * WN * 64;                // threads
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int MI = TM / 32, NI = TN / 32;
  constexpr int RPP = NT / KQ;                    // A rows staged per pass
  constexpr int AQ = BM / RPP;                    // A quads (4 k-values) staged per thread
  constexpr int BI = (BN * 2 * QB + NT - 1) / NT; // B 16-byte items staged per thread (hi+lo planes)
  static_assert(BM % RPP == 0, "A staging must tile the rows");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* As = smem;                       // [2][BM][ROWB]
  unsigned char* Bs = smem + gemm_off_b(BM, ROWB);   // [2][BN][ROWB]
  static_assert(gemm_patches_fit(BM, BN, ROWB, WM * WN), "the epilogues' 32 x 36 patches must fit in the idle staging ring");

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const int wr = wid / WN, wc = wid % WN;

  const int mtiles = (p.M + BM - 1) / BM, ntiles = (p.Cout + BN - 1) / BN;
  const int L = ff_xcd_remap(blockIdx.x, mtiles * ntiles);
  const int m0 = (L / ntiles) * BM, n0 = (L % ntiles) * BN;

  const int srow = tid / KQ, kq = tid % KQ;       // A staging: row srow + RPP*i, k-quad kq
  int a_b[AQ], a_iy[AQ], a_ix[AQ];
  bool a_ok[AQ];
#pragma unroll
  for (int i = 0; i < AQ; ++i) {
    const int m = m0 + srow + RPP * i;
    a_ok[i] = m < p.M;
    const int mm = a_ok[i] ? m : 0;
    const int ox = mm % p.Wo, t2 = mm / p.Wo;
    const int oy = t2 % p.Ho;
    a_b[i] = t2 / p.Ho;
    a_iy[i] = oy * p.sy - p.py;
    a_ix[i] = ox * p.sx - p.px;
  }
  const bool is1x1 = (p.KH == 1 && p.KW == 1);

  f32x4 ra[AQ];
  uint4 rb[BI];

  auto load_chunk = [&](int k0) {
    if (VEC4) {
      int ky = 0, kx = 0, ci;
      bool kok;
      if (p.Cp > 0) {                               // TAP mode: tap / ci0 are uniform (scalar) per chunk
        const int tap = k0 / p.Cp;
        ci = k0 - tap * p.Cp + 4 * kq;
        kok = ci < p.Cin;
        ky = tap / p.KW;
        kx = tap - ky * p.KW;
      } else {
        const int k = k0 + 4 * kq;
        kok = k < p.K;
        ci = k;
        if (!is1x1 && kok) {
          const int tap = k / p.Cin;
          ci = k - tap * p.Cin;
          ky = tap / p.KW;
          kx = tap - ky * p.KW;
        }
      }
#pragma unroll
      for (int i = 0; i < AQ; ++i) {
        const int iy = a_iy[i] + ky, ix = a_ix[i] + kx;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (kok && a_ok[i] && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
          v = *reinterpret_cast<const f32x4*>(p.in + ((long long)(a_b[i] * p.H + iy) * p.W + ix) * p.ldi + ci);
        ra[i] = v;
      }
#if CIG_KMUL_IMAGES
      if (kok) {                                      // kmul [B][Cin]: the image of each A row picks its vector (a_b < B also for rows beyond M)
#pragma unroll
        for (int i = 0; i < AQ; ++i) ra[i] *= *reinterpret_cast<const f32x4*>(p.kmul + (long long)a_b[i] * p.Cin + ci);
      }
#else
      if (p.kmul && kok) {                            // (1x1: ci is the input channel; the launcher checks Cin % 4 == 0)
        const f32x4 km = *reinterpret_cast<const f32x4*>(p.kmul + ci);
#pragma unroll
        for (int i = 0; i < AQ; ++i) ra[i] *= km;
      }
#endif
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + 4 * kq + e;
        const bool kok = k < p.K;
        int ky = 0, kx = 0, ci = k;
        if (!is1x1 && kok) {
          const int tap = k / p.Cin;
          ci = k - tap * p.Cin;
          ky = tap / p.KW;
          kx = tap - ky * p.KW;
        }
#pragma unroll
        for (int i = 0; i < AQ; ++i) {
          const int iy = a_iy[i] + ky, ix = a_ix[i] + kx;
          float v = 0.f;
          if (kok && a_ok[i] && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
            v = p.in[((long long)(a_b[i] * p.H + iy) * p.W + ix) * p.ldi + ci];
          ra[i][e] = v;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      const int id = tid + NT * j;                 // [plane][row][q]
      const int plane = id / (BN * QB), rem = id % (BN * QB);
      const int r = rem / QB, q = rem % QB;
      uint4 v = {0u, 0u, 0u, 0u};
      if (id < BN * 2 * QB && (NTERMS == 3 || plane == 0) && n0 + r < p.Cout) {
#if CIG_W_IMAGES
        const __bf16* src = (plane ? p.w_lo : p.w_hi) + ((long long)(m0 / p.W) * p.Cout + n0 + r) * p.Kp + k0 + 8 * q;
#else
        const __bf16* src = (plane ? p.w_lo : p.w_hi) + (long long)(n0 + r) * p.Kp + k0 + 8 * q;
#endif
        v = *reinterpret_cast<const uint4*>(src);
      }
      rb[j] = v;
    }
  };

  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AQ; ++i) {
      bf16x4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float f = ra[i][e];
        const __bf16 h = (__bf16)f;
        hi[e] = h;
        lo[e] = (__bf16)(f - (float)h);
      }
      unsigned char* dst = As + (size_t)(buf * BM + srow + RPP * i) * ROWB + kq * 8;
      *reinterpret_cast<bf16x4*>(dst) = hi;
      if (NTERMS >= 2) *reinterpret_cast<bf16x4*>(dst + PLB) = lo;
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      const int id = tid + NT * j;
      const int plane = id / (BN * QB), rem = id % (BN * QB);
      const int r = rem / QB, q = rem % QB;
      if (id < BN * 2 * QB && (NTERMS == 3 || plane == 0))
        *reinterpret_cast<uint4*>(Bs + (size_t)(buf * BN + r) * ROWB + plane * PLB + q * 16) = rb[j];
    }
  };

#include "gemm_acc_zero.inc"

  const int nchunks = p.Kp / BKB;
  load_chunk(0);
  store_chunk(0);
  __syncthreads();

  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) load_chunk((c + 1) * BKB);
#pragma unroll
    for (int s = 0; s < BKB / 16; ++s) {
      bf16x8 ah[MI], al[MI], bh[NI], bl[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const unsigned char* ap = As + (size_t)(buf * BM + wr * TM + i * 32 + l31) * ROWB + 32 * s + 16 * hh;
        ah[i] = *reinterpret_cast<const bf16x8*>(ap);
        if (NTERMS >= 2) al[i] = *reinterpret_cast<const bf16x8*>(ap + PLB);
      }
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const unsigned char* bp = Bs + (size_t)(buf * BN + wc * TN + j * 32 + l31) * ROWB + 32 * s + 16 * hh;
        bh[j] = *reinterpret_cast<const bf16x8*>(bp);
        if (NTERMS == 3) bl[j] = *reinterpret_cast<const bf16x8*>(bp + PLB);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          if (NTERMS == 3) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          if (NTERMS >= 2) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
    if (c + 1 < nchunks) store_chunk(buf ^ 1);
    __syncthreads();
  }

  auto epilogue = [&](auto ACTC) {
    constexpr int ACT = decltype(ACTC)::value;
    const bool has_res = p.res != nullptr;
    if (p.gate) {
      // SimpleGate (nafnet_arch.py:28-31, 100-104) on interleaved columns: the caller orders the weight rows so that the two halves of
      // the reference's chunk(2, dim=1) alternate (2j <- j, 2j+1 <- j + C); a lane then multiplies adjacent columns of the
      // transposed 32 x 32 tile and stores four consecutive product channels: the 2C-wide tensor never reaches memory.
      float* tr = reinterpret_cast<float*>(smem) + wid * (32 * 36);    // over the idle ring (asserted at the carve-up)
      const int grow = lane >> 2, seg = lane & 3;
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int n = n0 + wc * TN + j * 32 + l31;
        const float bv = (p.bias && n < p.Cout) ? p.bias[n] : 0.f;
        const int nq = (n0 + wc * TN + j * 32) / 2 + 4 * seg;      // first of this lane's four output channels
        const bool nqok = nq < p.Cout / 2;
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
            const int m = mb + row;
            if (nqok && m < p.M) *reinterpret_cast<f32x4*>(p.out + (long long)m * p.ldo + nq) = o;
          }
        }
      }
      return;
    }
    if (p.vec_out) {
      // 16-byte form: each 32(m) x 32(n) accumulator tile goes through a wave-private LDS patch (the staging buffers are
      // idle now) so a lane owns four consecutive channels of one row: float4 residual loads and stores, 8 whole
      // 128-byte row segments per instruction instead of 2 with dword accesses.
      float* tr = reinterpret_cast<float*>(smem) + wid * (32 * 36);    // over the idle ring (asserted at the carve-up)
      const int tq = lane >> 3, q4 = 4 * (lane & 7);
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int n = n0 + wc * TN + j * 32 + l31;
        const int nc = n < p.Cout ? n : 0;
        const float bv = p.bias ? p.bias[nc] : 0.f;
        const float mv = (p.mul ? p.mul[nc] : 1.f) * p.alpha;
        const int nq = n0 + wc * TN + j * 32 + q4;
        const bool nqok = nq < p.Cout;
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
          for (int r = 0; r < 16; ++r)
            tr[((r & 3) + 8 * (r >> 2) + 4 * hh) * 36 + l31] = ff_act_c<ACT, true>(acc[i][j][r] + bv) * mv;
          f32x4 ov[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) ov[k] = *reinterpret_cast<const f32x4*>(tr + (tq + 8 * k) * 36 + q4) + rq[k];
          if (nqok && mb + 32 <= p.M) {
#pragma unroll
            for (int k = 0; k < 4; ++k) *reinterpret_cast<f32x4*>(p.out + oo[k]) = ov[k];
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (ok[k]) *reinterpret_cast<f32x4*>(p.out + oo[k]) = ov[k];
          }
        }
      }
      return;
    }
#define CIG_ACT_FAST true
#include "conv_igemm_rows_epilogue.inc"
#undef CIG_ACT_FAST
  };
  FF_DISPATCH_ACT(p.act, epilogue)
}
