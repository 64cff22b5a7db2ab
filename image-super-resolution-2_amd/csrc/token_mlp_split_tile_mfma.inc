// One 32-row weight tile (hi + lo plane, W1B apart) times the wave's TM_KS fragment steps where the tokens' lo fragments lie in the
// wave's LDS rows: the loop of ff_tile_mfma (ff_common.h) with xl read from xl_row two steps ahead like the weights.  Shared as text (as a
// function it reorders the reads) by the projection of token_projmlp_kernel and the hidden-tile loop of token_mlp_split_tiles.inc.
// Expects ap, W1B, xh, xl_row, TM_NTERMS (1 or 3) and TM_ACC, the accumulator.
  bf16x8 fa[2], fl[2], fx[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    fa[u] = *reinterpret_cast<const bf16x8*>(ap + 32 * u);
    fl[u] = *reinterpret_cast<const bf16x8*>(ap + 32 * u + W1B);
    fx[u] = *reinterpret_cast<const bf16x8*>(xl_row + 32 * u);
  }
#pragma unroll
  for (int st = 0; st < TM_KS; ++st) {
    const bf16x8 ah = fa[st & 1], al = fl[st & 1], xl = fx[st & 1];
    if (st + 2 < TM_KS) {
      fa[st & 1] = *reinterpret_cast<const bf16x8*>(ap + 32 * (st + 2));
      fl[st & 1] = *reinterpret_cast<const bf16x8*>(ap + 32 * (st + 2) + W1B);
      fx[st & 1] = *reinterpret_cast<const bf16x8*>(xl_row + 32 * (st + 2));
    }
    __builtin_amdgcn_sched_barrier(0);
    if (TM_NTERMS == 3) {
      TM_ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xl, TM_ACC, 0, 0, 0);
      TM_ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, xh[st], TM_ACC, 0, 0, 0);
    }
    TM_ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xh[st], TM_ACC, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
