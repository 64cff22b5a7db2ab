// One 32-row weight tile (hi + lo plane, WB apart) times the wave's TL_KS fragment steps of token_linear_kernel: the loop of ff_tile_mfma
// (ff_common.h), shared as text by the kernel's gate GEMM and its main tile loop because through the function the main loop's operand
// reads change order and registers.  Expects ap, WB, NTERMS and TL_XH / TL_XL (the tokens' hi / lo fragments), TL_ACC (the accumulator).
  bf16x8 fa[2], fl[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    fa[u] = *reinterpret_cast<const bf16x8*>(ap + 32 * u);
    if (NTERMS == 3) fl[u] = *reinterpret_cast<const bf16x8*>(ap + 32 * u + WB);
  }
#pragma unroll
  for (int st = 0; st < TL_KS; ++st) {
    const bf16x8 ah = fa[st & 1], al = fl[st & 1];
    if (st + 2 < TL_KS) {
      fa[st & 1] = *reinterpret_cast<const bf16x8*>(ap + 32 * (st + 2));
      if (NTERMS == 3) fl[st & 1] = *reinterpret_cast<const bf16x8*>(ap + 32 * (st + 2) + WB);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (NTERMS == 3) {
      TL_ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, TL_XL[st], TL_ACC, 0, 0, 0);
      TL_ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, TL_XH[st], TL_ACC, 0, 0, 0);
    }
    TL_ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, TL_XH[st], TL_ACC, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
