// Projection of the plain-bf16 token_projmlp phase: the six proj^T tiles (bias as the MFMAs' C-in) into the output accumulators, from
// the LDS image of token_projmlp_bf16_dma.inc.  A statement sequence of token_projmlp_bf16_kernel, shared as text with hab_link.hip.
// Expects smem, xh, l31, hh and Bps, the padded projection bias in LDS (staged before the barrier that precedes this text: a global
// read here would make every tile wait for whatever loads the kernel has in flight -- the first residual slices); leaves oacc.
  f32x16 oacc[6];
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    const float* bpn = Bps + n * 32 + 4 * hh;
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[n][r] = bpn[(r & 3) + 8 * (r >> 2)];
    const unsigned char* ap = smem + n * PM_W1SLOT + l31 * W1ROWB + 16 * hh;
#define PM_ACC oacc[n]
#include "token_projmlp_bf16_tile_mfma.inc"
#undef PM_ACC
  }
