// One 32-row weight tile (hi plane only) times the wave's TM_KS fragment steps of the plain-bf16 token_projmlp phase: the loop of
// ff_tile_mfma<TM_KS, 1> (ff_common.h), shared as text by token_projmlp_bf16_proj.inc and token_projmlp_bf16_mlp.inc because through the
// function token_projmlp_bf16_kernel's address adds swap operands and the builds with phase stamps of both including kernels move.
// Expects ap, xh and PM_ACC, the accumulator.
  bf16x8 fa[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) fa[u] = *reinterpret_cast<const bf16x8*>(ap + 32 * u);
#pragma unroll
  for (int st = 0; st < TM_KS; ++st) {
    const bf16x8 ah = fa[st & 1];
    if (st + 2 < TM_KS) fa[st & 1] = *reinterpret_cast<const bf16x8*>(ap + 32 * (st + 2));
    __builtin_amdgcn_sched_barrier(0);
    PM_ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xh[st], PM_ACC, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
