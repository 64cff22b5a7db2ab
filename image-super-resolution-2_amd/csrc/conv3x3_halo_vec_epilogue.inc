// Vector epilogue of the LDS-resident 3x3 convolutions, shared as text by conv3x3_halo_kernel (conv3x3_halo.hip) and cab_fused_kernel
// (cab_fused.hip): bias + activation, the transposition through the wave's LDS patch, 16-byte stores and the per-workgroup pool partial row.
// The including scope provides p (res, mul, bias, alpha, out, ldo, ldr, io_bf16, pool_part, H, W, Cout), smem, acc[MI][NI], the wave's
// coordinates (wid, lane, l31, hh, wr, wc), the tile origin (b, y0, x0, n0) and the constants WM, WN, MI, NI, TN, BN, NT, NTERMS, ACT, TWO_PER_CU,
// and VEC_EPI_SPACE: the bytes from smem on that are idle staging in the epilogue.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                        // every wave has left the tap loop: the staging area is free
    float* ps = reinterpret_cast<float*>(smem);          // [WM][BN] pool partials below HALO_OFF_PATCH, then the waves' 32 x 36 patches
    float* patch = reinterpret_cast<float*>(smem + HALO_OFF_PATCH) + wid * (32 * 36);
    static_assert(halo_epilogue_fits(WM, WN, BN, VEC_EPI_SPACE), "pool row under HALO_OFF_PATCH, patches inside the idle staging");
    const int tq = lane >> 3, q4 = 4 * (lane & 7);
    const bool has_res = p.res != nullptr;
    // residual quads are requested one n-tile ahead of their use (fetched right before the add, each tile exposed an HBM latency: the
    // finding of sgfn_tail's epilogue; all tiles at once spills the big-accumulator forms)
    constexpr bool RES_AHEAD = !(TWO_PER_CU || (NTERMS == 1 && MI * NI <= 2 && WM * WN == 4));   // the 128- / 168-register forms fetch at use
    f32x4 rq[2][MI][4];
    auto load_res = [&](int j, f32x4 (&dst)[MI][4]) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int mrow = tq + 8 * k, c4 = n0 + wc * TN + j * 32 + q4;
          const int oy = y0 + (wr * MI + i) * 2 + (mrow >> 4), ox = x0 + (mrow & 15);
          const bool ok = c4 < p.Cout && oy < p.H && ox < p.W;
          dst[i][k] = ok ? *reinterpret_cast<const f32x4*>(p.res + ((long long)(b * p.H + oy) * p.W + ox) * p.ldr + c4) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    if (RES_AHEAD && has_res) load_res(0, rq[0]);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = n0 + wc * TN + j * 32 + l31;
      const bool nok = n < p.Cout;
      const float bv = (nok && p.bias) ? p.bias[n] : 0.f;
      const float mv = ((nok && p.mul) ? p.mul[n] : 1.f) * p.alpha;
      const int c4 = n0 + wc * TN + j * 32 + q4;         // the four channels this lane stores
      const bool cok = c4 < p.Cout;
      if (RES_AHEAD && has_res && j + 1 < NI) load_res(j + 1, rq[(j + 1) & 1]);
      f32x4 mv4 = {p.alpha, p.alpha, p.alpha, p.alpha};
      if (p.mul && cok) mv4 = *reinterpret_cast<const f32x4*>(p.mul + c4) * p.alpha;
      float psum = 0.f;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int ry0 = y0 + (wr * MI + i) * 2;
#pragma unroll
        for (int r = 0; r < 16; ++r) {                   // register r = tile row (r & 3) + 8 (r >> 2) + 4 hh of channel l31
          const int mrow = (r & 3) + 8 * (r >> 2) + 4 * hh;
          const float a = ff_act_c<ACT, true>(acc[i][j][r] + bv);
          patch[mrow * 36 + l31] = a;                      // scale and residual are applied after the transposition, as one fma (the scalar path's rounding)
          if (nok && ry0 + (mrow >> 4) < p.H && x0 + (mrow & 15) < p.W) psum += a * mv;  // (pool partials: no residual on this path)
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int mrow = tq + 8 * k;
          const int oy = ry0 + (mrow >> 4), ox = x0 + (mrow & 15);
          const bool ok = cok && oy < p.H && ox < p.W;
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(patch + mrow * 36 + q4);
          const long long pix = ok ? ((long long)(b * p.H + oy) * p.W + ox) : 0;
          f32x4 r4 = {0.f, 0.f, 0.f, 0.f};
          if (RES_AHEAD && has_res) r4 = rq[j & 1][i][k];
          else if (has_res && ok) r4 = *reinterpret_cast<const f32x4*>(p.res + pix * p.ldr + c4);
          f32x4 v4;
#pragma unroll
          for (int e = 0; e < 4; ++e) v4[e] = __builtin_fmaf(a4[e], mv4[e], r4[e]);
          if (ok) {
            if (NTERMS == 1 && (p.io_bf16 & 2)) {
              bf16x4 h4;
#pragma unroll
              for (int e = 0; e < 4; ++e) h4[e] = (__bf16)v4[e];
              *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(p.out) + pix * p.ldo + c4) = h4;
            } else {
              *reinterpret_cast<f32x4*>(p.out + pix * p.ldo + c4) = v4;
            }
          }
        }
      }
      if (p.pool_part) {
        psum += __shfl_xor(psum, 32);
        if (hh == 0) ps[wr * BN + wc * TN + j * 32 + l31] = psum;
      }
    }
    if (p.pool_part) {
      __syncthreads();
      for (int c = threadIdx.x; c < BN; c += NT) {
        float sacc = 0.f;
#pragma unroll
        for (int w = 0; w < WM; ++w) sacc += ps[w * BN + c];
        p.pool_part[(long long)blockIdx.x * BN + c] = sacc;
      }
    }
