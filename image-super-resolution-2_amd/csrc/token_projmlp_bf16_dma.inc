// LDS-DMA of the plain-bf16 token_projmlp phase: the whole projection image, issued here, and the slot maps of the MLP's double-buffered
// W1 / W2 tiles.  A statement sequence of token_projmlp_bf16_kernel, shared as text with hab_link.hip.  Expects smem, wid, lane and
// PM_P(f), the including kernel's name for field f of TokenProjMlpParams (wp, w); leaves off1, off2 and dma_mlp(ht, slot).
  // ---- the whole projection (6 tiles x 13 one-KiB pieces, hi plane) by LDS-DMA ----------------------------------------------
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const int pc = wid + 8 * i;
    if (pc < 78) {
      const int tile = pc / 13, pw = pc - 13 * tile;
      int s = pw * 64 + lane;
      if (s > W1PL - 1) s = W1PL - 1;
      const int row = s / W1SLOTS;
      int q = s - row * W1SLOTS;
      if (q > 23) q = 23;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(PM_P(wp) + (long long)tile * (2 * TILE_ELEMS) + row * 192 + q * 8),
                                       (__attribute__((address_space(3))) void*)(smem + pc * 1024), 16, 0, 0);
    }
  }
  int off1[2], off2[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int s = (wid + 8 * i) * 64 + lane;
    if (s > W1PL - 1) s = W1PL - 1;
    int row = s / W1SLOTS, q = s - row * W1SLOTS;
    if (q > 23) q = 23;
    off1[i] = row * 192 + q * 8;
    s = (wid + 8 * i) * 64 + lane;
    if (s > W2PL - 1) s = W2PL - 1;
    row = s / W2SLOTS; q = s - row * W2SLOTS;
    if (q > 3) q = 3;
    off2[i] = 2 * TILE_ELEMS + row * 32 + q * 8;
  }
  auto dma_mlp = [&](int ht, int slot) {
    const __bf16* rec = PM_P(w) + (long long)ht * (4 * TILE_ELEMS);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (wid + 8 * i < 13)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rec + off1[i]),
                                         (__attribute__((address_space(3))) void*)(smem + slot * PM_W1SLOT + (wid + 8 * i) * 1024), 16, 0, 0);
      if (wid + 8 * i < 15)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(rec + off2[i]),
                                         (__attribute__((address_space(3))) void*)(smem + PM_OFF_W2 + slot * PM_W2SLOT + (wid + 8 * i) * 1024), 16, 0, 0);
    }
  };
