// LayerNorm statistics of x1 taken from the output accumulators (a lane holds 96 of its token's 192 padded channels, lane + 32 the other
// half): a statement sequence shared as text by token_projmlp_kernel (token_mlp.hip), token_projmlp_bf16_ln.inc and through it
// token_projmlp_bf16_kernel and hab_link_kernel; the reduction order is part of the result.  Expects oacc, hh, p.K and PM_P(f), the
// including kernel's name for field f of TokenProjMlpParams (eps); leaves mean and rstd in the includer's block.
    // inline on purpose: through a shared helper (by reference, by value or returning a struct alike) token_projmlp_kernel spills
    // 28-31 VGPRs (116-128 B of scratch) and token_projmlp_bf16_kernel 6-12 (28-52 B); as written here neither spills
    float s = 0.f;
#pragma unroll
    for (int n = 0; n < 6; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) s += (n * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh < p.K) ? oacc[n][r] : 0.f;
    s += __shfl_xor(s, 32);
    const float mean = s / (float)p.K;
    float qv = 0.f;
#pragma unroll
    for (int n = 0; n < 6; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float d = (n * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh < p.K) ? oacc[n][r] - mean : 0.f;
        qv += d * d;
      }
    qv += __shfl_xor(qv, 32);
    const float rstd = 1.0f / sqrtf(qv / (float)p.K + PM_P(eps));
