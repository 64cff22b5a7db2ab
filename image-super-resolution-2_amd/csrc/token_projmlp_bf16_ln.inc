// LayerNorm(x1) from the output accumulators -> fc1's bf16 operand fragments: a statement sequence of token_projmlp_bf16_kernel,
// shared as text with hab_link.hip.  Expects oacc, xh, hh, Gs / Bts (gamma / beta in LDS, zero padded to 192), p.K and PM_P(f) (eps).
  {
#include "token_projmlp_ln_stats.inc"
#pragma unroll
    for (int n = 0; n < 6; ++n)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
        for (int g2 = 0; g2 < 2; ++g2) {
          const int c0 = n * 32 + 8 * (2 * s2 + g2) + 4 * hh;           // channels of registers 8 s2 + 4 g2 .. + 3 (< 192: the vectors are zero padded)
          const f32x4 g4 = *reinterpret_cast<const f32x4*>(Gs + c0);
          const f32x4 b4 = *reinterpret_cast<const f32x4*>(Bts + c0);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            xh[2 * n + s2][4 * g2 + e] = (__bf16)((oacc[n][8 * s2 + 4 * g2 + e] - mean) * rstd * g4[e] + b4[e]);
        }
        // the fragment is pinned here: left to itself the scheduler issues all 48 vector reads first and sinks the arithmetic
        // below them (192 live registers, 52 of them spilled)
        asm volatile("" : "+v"(xh[2 * n + s2]) :: "memory");
      }
  }
