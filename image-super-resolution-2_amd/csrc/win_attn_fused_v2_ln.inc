// LayerNorm of the fragment rows v[][] -> bf16 operand fragments xh[] (+ the normalised side output): a statement sequence of
// win_attn_fused_v2_kernel, shared as text with hab_link.hip (the reduction order is part of the result).  Expects p (gamma, beta, K, eps, xn, xn_bf16,
// ldxn), v, xh, hh, mytok, tvalid, and W2_LN(f): where the vector f (gamma, beta) is read from -- p.f in the stand-alone kernels, an LDS
// copy in hab_link.hip, whose LayerNorm runs while every workgroup's x_out stores are in flight (p.gamma stays the "has a norm" test).
    // ff_frag_ln_stats, inline on purpose: with the helper every instantiation goes from 171 / 196 to 246 VGPRs and
    // win_attn_fused_v2_kernel<32, true> from 46.17 / 45.91 us to 46.36 / 47.23 us under the bench
    float mean = 0.f, rstd = 1.f;
    if (p.gamma) {
      float s = 0.f;
#pragma unroll
      for (int st = 0; st < WF_KS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[st][j];
      s += __shfl_xor(s, 32);
      mean = s / (float)p.K;
      // corrected two-pass: the residuals' own sum repairs the rounding of the first-pass mean.  On a (near-)constant row that rounding
      // is all there is -- 0.1 in every channel came out 8.8e-6 from beta, (x - mean) * rstd with rstd = 316 -- and x - mean is exact.
      float qv = 0.f, sd = 0.f;
#pragma unroll
      for (int st = 0; st < WF_KS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float dd = (16 * st + 8 * hh + j < p.K) ? v[st][j] - mean : 0.f;
          qv += dd * dd;
          sd += dd;
        }
      qv += __shfl_xor(qv, 32);
      sd += __shfl_xor(sd, 32);
      const float dm = sd / (float)p.K;
      mean += dm;
      rstd = 1.0f / sqrtf(fmaxf(qv / (float)p.K - dm * dm, 0.f) + p.eps);
    }
#pragma unroll
    for (int st = 0; st < WF_KS; ++st) {
      const int k0 = 16 * st + 8 * hh;
      f32x4 g0 = {1.f, 1.f, 1.f, 1.f}, g1 = g0, b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
      if (p.gamma) {
        const int ka = k0 < p.K ? k0 : 0, kb = k0 + 4 < p.K ? k0 + 4 : 0;
        g0 = *reinterpret_cast<const f32x4*>(W2_LN(gamma) + ka); b0 = *reinterpret_cast<const f32x4*>(W2_LN(beta) + ka);
        g1 = *reinterpret_cast<const f32x4*>(W2_LN(gamma) + kb); b1 = *reinterpret_cast<const f32x4*>(W2_LN(beta) + kb);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gg = j < 4 ? g0[j & 3] : g1[j & 3], bb = j < 4 ? b0[j & 3] : b1[j & 3];
        const float f = (k0 + j < p.K) ? (p.gamma ? (v[st][j] - mean) * rstd * gg + bb : v[st][j]) : 0.f;
        xh[st][j] = (__bf16)f;
        v[st][j] = f;
      }
      if (p.xn && tvalid && p.xn_bf16) {             // bf16 side output: the fragment itself (its consumer rounds to bf16 anyway)
        if (k0 < p.K) *reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(p.xn) + (long long)mytok * p.ldxn + k0) = xh[st];
      } else if (p.xn && tvalid) {
        float* xr = p.xn + (long long)mytok * p.ldxn + k0;
        if (k0 < p.K) *reinterpret_cast<f32x4*>(xr) = (f32x4){v[st][0], v[st][1], v[st][2], v[st][3]};
        if (k0 + 4 < p.K) *reinterpret_cast<f32x4*>(xr + 4) = (f32x4){v[st][4], v[st][5], v[st][6], v[st][7]};
      }
    }
