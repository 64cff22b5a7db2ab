// Hidden-tile loop of the split-bf16 token MLP (fc1 tile, GELU + split, fc2 accumulation; two barriers per tile), shared as text by
// token_mlp_kernel and token_projmlp_kernel (token_mlp.hip includes this file twice).  Expects p.HT, W1s, W2s, W1B, W2B, B1s, xh, xl_row,
// oacc, l31, hh, dma_w1, dma_w2 (token_mlp_split_dma.inc), TM_NTERMS (1 or 3: 1 drops the two lo-term MFMAs of every step) and
// TM_STAMP(i), the including kernel's phase stamp (an empty statement where the kernel has none).
  for (int ht = 0; ht < p.HT; ++ht) {
    // ---- H^T tile = b1 + W1 . LN(x)^T ------------------------------------------------------------------------
    f32x16 hacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) hacc[r] = B1s[ht * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh];
    {
      const unsigned char* ap = W1s + l31 * W1ROWB + 16 * hh;
#define TM_ACC hacc
#include "token_mlp_split_tile_mfma.inc"
#undef TM_ACC
    }
    if (ht < 3) TM_STAMP(8 + 4 * ht);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // W2(ht) pieces of this wave have landed
    __syncthreads();                                    // A: every wave finished reading W1; W2(ht) visible to all
    if (ht < 3) TM_STAMP(9 + 4 * ht);
    if (ht + 1 < p.HT) dma_w1(ht + 1);
    // ---- GELU, split; registers 8s..8s+7 are the B fragment of k-step s ----------------------------------------
    bf16x8 gh[2], gl[2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = ff_gelu_fast(hacc[8 * s + j]);
        const __bf16 h = (__bf16)g;
        gh[s][j] = h;
        gl[s][j] = (__bf16)(g - (float)h);
      }
    // ---- OUT^T += W2 . H^T ---------------------------------------------------------------------------------------
    {
      const unsigned char* ap = W2s + l31 * W2ROWB + 16 * hh;        // step u = 2n + s: row n*32 + l31, k-step s
      bf16x8 fa[2], fl[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        fa[u] = *reinterpret_cast<const bf16x8*>(ap + (u >> 1) * 32 * W2ROWB + 32 * (u & 1));
        fl[u] = *reinterpret_cast<const bf16x8*>(ap + (u >> 1) * 32 * W2ROWB + 32 * (u & 1) + W2B);
      }
#pragma unroll
      for (int u = 0; u < 12; ++u) {
        const int n = u >> 1, s2 = u & 1;
        const bf16x8 ah = fa[u & 1], al = fl[u & 1];
        if (u + 2 < 12) {
          fa[u & 1] = *reinterpret_cast<const bf16x8*>(ap + ((u + 2) >> 1) * 32 * W2ROWB + 32 * ((u + 2) & 1));
          fl[u & 1] = *reinterpret_cast<const bf16x8*>(ap + ((u + 2) >> 1) * 32 * W2ROWB + 32 * ((u + 2) & 1) + W2B);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (TM_NTERMS == 3) {
          oacc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, gl[s2], oacc[n], 0, 0, 0);
          oacc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, gh[s2], oacc[n], 0, 0, 0);
        }
        oacc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, gh[s2], oacc[n], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (ht < 3) TM_STAMP(10 + 4 * ht);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // W1(ht+1) pieces of this wave have landed
    __syncthreads();                                    // B: every wave finished reading W2; W1(ht+1) visible to all
    if (ht < 3) TM_STAMP(11 + 4 * ht);
    if (ht + 1 < p.HT) dma_w2(ht + 1);
  }
