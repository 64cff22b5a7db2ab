// The optional-gamma LayerNorm step on MFMA B fragments, with the side output of the normalised rows: ff_frag_ln_step (ff_common.h) where
// gamma may be absent (the rows then pass through), the bf16 split, and xn[token] = the normalised row.  Shared as text by
// win_attn_fused_kernel and token_linear_kernel (the statistics helper already costs the latter an occupancy step; see ff_common.h).
// Side output (HAT feeds the normalised rows to the CAB convolution, hat_arch.py:272-274): the separate LayerNorm pass (read 47 MB, write
// 47 MB) becomes 47 MB of extra stores here.  A lane holds 8 consecutive channels of its row: two float4 stores; the 12 steps of a wave
// complete whole lines in L2 before they are evicted.
// Expects p (gamma, beta, K, xn, ldxn), v, mean, rstd, xh, xl, hh, tvalid, NTERMS and LN_OPT_KS (the k-steps), LN_OPT_TOK (the lane's
// token index as a long long).
#pragma unroll
    for (int st = 0; st < LN_OPT_KS; ++st) {
      const int k0 = 16 * st + 8 * hh;
      f32x4 g0 = {1.f, 1.f, 1.f, 1.f}, g1 = g0, b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
      if (p.gamma) {
        const int ka = k0 < p.K ? k0 : 0, kb = k0 + 4 < p.K ? k0 + 4 : 0;
        g0 = *reinterpret_cast<const f32x4*>(p.gamma + ka); b0 = *reinterpret_cast<const f32x4*>(p.beta + ka);
        g1 = *reinterpret_cast<const f32x4*>(p.gamma + kb); b1 = *reinterpret_cast<const f32x4*>(p.beta + kb);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gg = j < 4 ? g0[j & 3] : g1[j & 3], bb = j < 4 ? b0[j & 3] : b1[j & 3];
        const float f = (k0 + j < p.K) ? (p.gamma ? (v[st][j] - mean) * rstd * gg + bb : v[st][j]) : 0.f;
        const __bf16 h = (__bf16)f;
        xh[st][j] = h;
        if (NTERMS == 3) xl[st][j] = (__bf16)(f - (float)h);
        v[st][j] = f;
      }
      if (p.xn && tvalid) {
        float* xr = p.xn + LN_OPT_TOK * p.ldxn + k0;
        if (k0 < p.K) *reinterpret_cast<f32x4*>(xr) = (f32x4){v[st][0], v[st][1], v[st][2], v[st][3]};
        if (k0 + 4 < p.K) *reinterpret_cast<f32x4*>(xr + 4) = (f32x4){v[st][4], v[st][5], v[st][6], v[st][7]};
      }
    }
