// Dword epilogue of the implicit-GEMM kernels (lane = output channel, registers = output pixels; plain rows or the 2x pixel shuffle),
// shared as text by conv_igemm_kernel (conv_gemm.hip) and conv_igemm_bf16_kernel.inc.  Expects p (ConvParams / ConvBfParams: out, res,
// bias, mul, alpha, M, Cout, ldo, ldr, shuffle, Ho, Wo), acc, ACT, has_res, m0, n0, wr, wc, TM, TN, MI, NI, l31, hh and
// CIG_ACT_FAST, the second argument of ff_act_c (false in the fp32 kernel, true in the bf16 ones).
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = n0 + wc * TN + j * 32 + l31;
      if (n >= p.Cout) continue;
      const float bv = p.bias ? p.bias[n] : 0.f;
      const float mv = (p.mul ? p.mul[n] : 1.f) * p.alpha;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        // indices first, then ALL residual loads, then the stores: `out` may alias `res` as far as the compiler knows,
        // so a residual load placed after a store is serialised behind it (16 dependent L2 round trips per tile)
        long long oidx[16];
        float rv[16];
        const int mb = m0 + wr * TM + i * 32 + 4 * hh;
        if (p.shuffle == 2) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = mb + (r & 3) + 8 * (r >> 2);
            const int mm = m < p.M ? m : 0;
            const int ox = mm % p.Wo, t2 = mm / p.Wo;
            const int oy = t2 % p.Ho, b = t2 / p.Ho;
            const int co = n >> 2, dy = (n >> 1) & 1, dx = n & 1;
            const long long pix = ((long long)(b * 2 * p.Ho + 2 * oy + dy) * (2 * p.Wo) + 2 * ox + dx);
            oidx[r] = pix * p.ldo + co;
            rv[r] = has_res ? p.res[pix * p.ldr + co] : 0.f;
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = mb + (r & 3) + 8 * (r >> 2);
            const int mm = m < p.M ? m : 0;
            oidx[r] = (long long)mm * p.ldo + n;
            rv[r] = has_res ? p.res[(long long)mm * p.ldr + n] : 0.f;
          }
        }
        if (mb + 28 < p.M) {                      // whole 32-row tile in range: no per-store exec masking
#pragma unroll
          for (int r = 0; r < 16; ++r) p.out[oidx[r]] = ff_act_c<ACT, CIG_ACT_FAST>(acc[i][j][r] + bv) * mv + rv[r];
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = mb + (r & 3) + 8 * (r >> 2);
            if (m < p.M) p.out[oidx[r]] = ff_act_c<ACT, CIG_ACT_FAST>(acc[i][j][r] + bv) * mv + rv[r];
          }
        }
      }
    }
