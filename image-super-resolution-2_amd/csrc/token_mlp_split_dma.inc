// LDS-DMA slot maps of the split-bf16 token MLP (W1 / W2 tile images, hi + lo planes), shared as text by token_mlp_kernel and
// token_projmlp_kernel (token_mlp.hip includes this file twice).  Expects p.w, W1s, W2s, wid, lane; leaves off1, off2, dma_w1, dma_w2.
  // ---- LDS-DMA bookkeeping: this wave fills pieces wid, wid+8, ... of each image; per lane the source offset in a tile record
  int off1[4], off2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int s = (wid + 8 * i) * 64 + lane;               // slot in the W1 image (2 planes x 32 rows x 25 slots)
    if (s >= 2 * W1PL) s = 2 * W1PL - 1;
    int plane = s / W1PL, t = s - plane * W1PL, row = t / W1SLOTS, q = t - row * W1SLOTS;
    if (q > 23) q = 23;
    off1[i] = plane * TILE_ELEMS + row * 192 + q * 8;
    s = (wid + 8 * i) * 64 + lane;                   // slot in the W2 image (2 planes x 192 rows x 5 slots)
    if (s >= 2 * W2PL) s = 2 * W2PL - 1;
    plane = s / W2PL; t = s - plane * W2PL; row = t / W2SLOTS; q = t - row * W2SLOTS;
    if (q > 3) q = 3;
    off2[i] = (2 + plane) * TILE_ELEMS + row * 32 + q * 8;
  }
  auto dma_w1 = [&](int ht) {
    const __bf16* rec = p.w + (long long)ht * (4 * TILE_ELEMS);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (wid + 8 * i < W1PIECES)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rec + off1[i]),
                                         (__attribute__((address_space(3))) void*)(W1s + (wid + 8 * i) * 1024), 16, 0, 0);
  };
  auto dma_w2 = [&](int ht) {
    const __bf16* rec = p.w + (long long)ht * (4 * TILE_ELEMS);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (wid + 8 * i < W2PIECES)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rec + off2[i]),
                                         (__attribute__((address_space(3))) void*)(W2s + (wid + 8 * i) * 1024), 16, 0, 0);
  };
