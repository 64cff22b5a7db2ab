// LayerNorm statistics of the NAFNet kernels on MFMA B fragments: ff_frag_ln_stats (ff_common.h) where the channel count C = 16 KS is a
// compile-time constant, so no k < K mask.  Shared as text by naf_front_kernel, naf_ffn_kernel and naf_tail_kernel: each measured slower
// (or moved its output bits) through the helper, see the comment at the including site.  Expects v[KS][8], C, p.eps; leaves mean, rstd.
    float s = 0.f;
#pragma unroll
    for (int st = 0; st < KS; ++st)
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[st][j];
    s += __shfl_xor(s, 32);
    const float mean = s / (float)C;
    float qv = 0.f;
#pragma unroll
    for (int st = 0; st < KS; ++st)
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = v[st][j] - mean; qv += d * d; }
    qv += __shfl_xor(qv, 32);
    const float rstd = 1.0f / sqrtf(qv / (float)C + p.eps);
