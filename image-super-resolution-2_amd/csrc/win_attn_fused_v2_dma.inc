// Per-head LDS-DMA map of win_attn_fused_v2_kernel: a head's weight image (38 one-KiB pieces, 5 per wave) and its bias table
// (<= 10 pieces), shared as text with hab_link.hip.  Expects smem, wid, lane and p (w, rel, rel_rows, rel_stride); leaves woff, reln,
// relpieces and dma_head(head, buf), which win_attn_fused_v2_heads.inc calls.
  int woff[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    int s = (wid + 8 * i) * 64 + lane;
    if (s >= W2_HEAD_SLOTS) s = W2_HEAD_SLOTS - 1;
    const int tile = s / WF_PL, t = s - tile * WF_PL, row = t / WF_SLOTS;
    int q = t - row * WF_SLOTS;
    if (q > 2 * WF_KS - 1) q = 2 * WF_KS - 1;
    woff[i] = tile * (2 * WF_TILE_ELEMS) + row * 192 + q * 8;
  }
  const int reln = p.rel_rows * p.rel_stride;           // floats per head table (a multiple of 4)
  const int relpieces = (reln + 255) >> 8;
  auto dma_head = [&](int head, int buf) {
    const __bf16* rec = p.w + (long long)(3 * head) * (2 * WF_TILE_ELEMS);
#pragma unroll
    for (int i = 0; i < 5; ++i)
      if (wid + 8 * i < W2_PIECES)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rec + woff[i]),
                                         (__attribute__((address_space(3))) void*)(smem + (wid + 8 * i) * 1024), 16, 0, 0);
    const float* src = p.rel + (long long)head * reln;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (wid + 8 * i < relpieces) {
        int c = (wid + 8 * i) * 64 + lane;
        if (c > (reln >> 2) - 1) c = (reln >> 2) - 1;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 4 * c),
                                         (__attribute__((address_space(3))) void*)(smem + W2_OFF_REL + buf * W2_RELB + WF_REL_PAD * 4 + (wid + 8 * i) * 1024), 16, 0, 0);
      }
  };
