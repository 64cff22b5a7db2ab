// Hidden-tile loop of token_projmlp_bf16_kernel (fc1 tile, GELU, fc2 accumulation; W1 / W2 double buffered), shared as text with
// hab_link.hip.  Expects smem, p.HT, B1s, xh, oacc, l31, hh, dma_mlp and PM_STAMP(i), the including kernel's phase stamp.
  // ---- the MLP over hidden tiles ---------------------------------------------------------------------------------------------
  for (int ht = 0; ht < p.HT; ++ht) {
    const int slot = ht & 1;
    f32x16 hacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) hacc[r] = B1s[ht * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh];
    {
      const unsigned char* ap = smem + slot * PM_W1SLOT + l31 * W1ROWB + 16 * hh;
#define PM_ACC hacc
#include "token_projmlp_bf16_tile_mfma.inc"
#undef PM_ACC
    }
    if (ht < 3) PM_STAMP(8 + 4 * ht);
    bf16x8 gh[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const f32x2 g = ff_gelu_sig2((f32x2){hacc[8 * s + j], hacc[8 * s + j + 1]});
        gh[s][j] = (__bf16)g[0];
        gh[s][j + 1] = (__bf16)g[1];
      }
    if (ht < 3) PM_STAMP(9 + 4 * ht);
    {
      const unsigned char* ap = smem + PM_OFF_W2 + slot * PM_W2SLOT + l31 * W2ROWB + 16 * hh;
      bf16x8 fa[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) fa[u] = *reinterpret_cast<const bf16x8*>(ap + (u >> 1) * 32 * W2ROWB + 32 * (u & 1));
#pragma unroll
      for (int u = 0; u < 12; ++u) {
        const int n = u >> 1, s2 = u & 1;
        const bf16x8 ah = fa[u & 1];
        if (u + 2 < 12) fa[u & 1] = *reinterpret_cast<const bf16x8*>(ap + ((u + 2) >> 1) * 32 * W2ROWB + 32 * ((u + 2) & 1));
        __builtin_amdgcn_sched_barrier(0);
        oacc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, gh[s2], oacc[n], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (ht < 3) PM_STAMP(10 + 4 * ht);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                        // every wave is done with this slot; tile ht+1 has landed everywhere
    if (ht < 3) PM_STAMP(11 + 4 * ht);
    if (ht + 2 < p.HT) dma_mlp(ht + 2, slot);
  }
