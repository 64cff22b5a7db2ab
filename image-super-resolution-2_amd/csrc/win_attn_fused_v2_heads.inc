// Per-head loop of win_attn_fused_v2_kernel (q / k / v tiles, online-softmax attention, O^T stores), shared as text with hab_link.hip.
// Expects the kernel's locals (smem, Bs, ktok, same, xh, qi, mytok, tvalid, qreg_id, vmask, kill_pad, msy, msx, blk_mask, dma_head, the
// WW / WH / RS / TPR / WWM / ONES constants) and W2_STAMP(i), the including kernel's phase stamp.
  // bias[q][k] = T[(qy - ky + WH-1) RS + (qx - kx + WW-1)].  Register r of a lane holds key 32 t + 31 - c of tile t,
  // c = (r & 3) + 8 (r >> 2) + 4 hh, so the index is (lane part) - (tile part) + (c / WW) RS + (c % WW): ascending in r
  const int rel_lane = ((qi / WW) + WH - 1) * RS + (qi % WW) + WW - 1 - (TPR - 1) * RS - (WWM - 1) + 4 * hh;
  const float LOG2E = 1.4426950408889634f;

  auto gemm_tile = [&](int j, bool swap, f32x16& acc) {
    const unsigned char* ap = smem + j * W2_TILEB + l31 * WF_ROWB + 16 * hh;
    ff_tile_mfma<WF_KS, 1>(ap, 0, xh, xh, swap, acc);
  };

  for (int hi = 0; hi < p.nheads; ++hi) {
    const int g = p.head0 + hi, buf = hi & 1;
    unsigned char* KB = smem + W2_OFF_K + buf * W2_KBUF;
    unsigned char* VB = smem + W2_OFF_V + buf * W2_VBUF;
    // every wave has confirmed its DMA pieces of this head (vmcnt(0) above / at the end of the previous attention) and is
    // past the previous head's attention
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    W2_STAMP(3 + 8 * hi);
    // ---- q tile: stays in registers ----------------------------------------------------------------------------------------
    bf16x8 qh[2];
    {
      f32x16 acc;
      const int nb = (3 * hi) * 32 + 4 * hh;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = Bs[nb + (r & 3) + 8 * (r >> 2)];
      gemm_tile(0, false, acc);
      if (ONES && blk_mask && hh) { acc[14] = msy; acc[15] = msx; }
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) qh[s][j] = (__bf16)acc[8 * s + j];
    }
    W2_STAMP(4 + 8 * hi);
    // ---- k tile -> K[key][d-permuted] ----------------------------------------------------------------------------------------
    {
      f32x16 acc;
      const int nb = (3 * hi + 1) * 32 + 4 * hh;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = Bs[nb + (r & 3) + 8 * (r >> 2)];
      gemm_tile(1, false, acc);
      const bool zero = kill_pad && !tvalid;
      if (zero) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      }
      if (ONES && blk_mask && hh) { acc[14] = msy; acc[15] = msx; }       // after the zeroing: padded keys keep their region
      unsigned char* kmine = KB + wid * W2_KWAVE + l31 * W2_KROWB + 16 * hh;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 h8;
#pragma unroll
        for (int j = 0; j < 8; ++j) h8[j] = (__bf16)acc[8 * s + j];
        *reinterpret_cast<bf16x8*>(kmine + 32 * s) = h8;
      }
    }
    W2_STAMP(5 + 8 * hi);
    // ---- v tile (operands swapped: lane = channel) -> V^T[d][key-permuted] (+ optional side output) --------------------------
    {
      f32x16 acc;
      const float bv = Bs[(3 * hi + 2) * 32 + l31];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = bv;
      gemm_tile(2, true, acc);
      if (kill_pad && !(ONES && l31 == 30)) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!((vmask >> ((r & 3) + 8 * (r >> 2) + 4 * hh)) & 1u)) acc[r] = 0.f;
      }
      unsigned char* vp = VB + l31 * W2_VROWB + 64 * wid + 16 * hh;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 h8;
#pragma unroll
        for (int j = 0; j < 8; ++j) h8[j] = (__bf16)acc[8 * s + j];
        *reinterpret_cast<bf16x8*>(vp + 32 * s) = h8;
      }
      if (p.vout && l31 < p.d) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int tk = ktok[wid * 32 + 31 - ((r & 3) + 8 * (r >> 2) + 4 * hh)];
          if (tk >= 0) p.vout[(long long)tk * p.ldv + p.v_off + g * p.d + l31] = acc[r];
        }
      }
    }
    W2_STAMP(6 + 8 * hi);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // K and V^T of this head are complete; every wave is done with the weight image
    W2_STAMP(7 + 8 * hi);
    if (hi + 1 < p.nheads) dma_head(g + 1, buf ^ 1);   // lands while the attention below runs

    // ---- attention: 8 tiles of 32 keys, online softmax -------------------------------------------------------------------------
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    unsigned rel_addr = (unsigned)(size_t)(__attribute__((address_space(3))) const void*)(smem + W2_OFF_REL + buf * W2_RELB + WF_REL_PAD * 4) + 4u * (unsigned)rel_lane;
    const unsigned char* kp = KB + l31 * W2_KROWB + 16 * hh;
    const unsigned char* vq = VB + l31 * W2_VROWB + 16 * hh;
    const unsigned* samep = same + 8 * qreg_id;
#pragma unroll 2
    for (int t = 0; t < 8; ++t, rel_addr -= 4u * TPR * RS, kp += W2_KWAVE, vq += 64) {
      unsigned ra = rel_addr;
      asm volatile("" : "+v"(ra));                      // one base register per tile: the 16 gathers below use immediates
      const ff_lds_cf relp = (ff_lds_cf)(size_t)ra;
      f32x16 st;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = (r & 3) + 8 * (r >> 2);
        st[r] = relp[(c / WW) * RS + (c % WW)];
      }
      bf16x8 vh2[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) vh2[s] = *reinterpret_cast<const bf16x8*>(vq + 32 * s);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(kp + 32 * s);
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, qh[s], st, 0, 0, 0);
      }
      if (!ONES && blk_mask) {
        const unsigned m = samep[t] >> (4 * hh);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          st[r] += ((m >> ((r & 3) + 8 * (r >> 2))) & 1u) ? 0.f : -100.0f;
      }
      float mx = st[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
      {
        float lo, hi;
        ff_halves(mx, lo, hi);
        mx = fmaxf(lo, hi);
      }
      if (__builtin_amdgcn_ballot_w64(mx > m_run) != 0) {          // some query's maximum moves: rescale (wave-uniform branch)
        const float m_new = fmaxf(m_run, mx);
        const float corr = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] *= corr;
        if (!ONES) l_run *= corr;
        m_run = m_new;
      }
      const float mneg = -m_run * LOG2E;
      float ls = 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 ph;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(st[8 * s + j], LOG2E, mneg));
          if (!ONES) ls += e;
          ph[j] = (__bf16)e;
        }
        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh2[s], ph, o, 0, 0, 0);
      }
      if (!ONES) l_run += ls;
    }
    float den;
    if (ONES) {                                          // channel 30 = register 14 of the upper half-wave holds the row sum of P
      float lo;
      ff_halves(o[14], lo, den);
    } else {
      den = l_run + __shfl_xor(l_run, 32);
    }
    const float inv = 1.0f / den;
    W2_STAMP(8 + 8 * hi);
    // the next head's DMA (issued ~an attention ago) and the side-output stores have landed: confirmed here, BEFORE this
    // head's output stores enter the queue, so that no later wait has to drain them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    W2_STAMP(9 + 8 * hi);

    // ---- O^T: lane = token, registers = channels, so every lane writes its own row segment directly (eight 8-byte stores
    //      at immediate offsets from one row pointer; the stores drain while the next head is projected) ----------------------
    if (tvalid && p.out_bf16) {
      typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
      __bf16* orow = reinterpret_cast<__bf16*>(p.out) + (long long)mytok * p.ldo + p.o_off + g * p.d + 4 * hh;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 8 * i + 4 * hh;
        if (c < p.d) *reinterpret_cast<bf16x2*>(orow + 8 * i) = (bf16x2){(__bf16)(o[4 * i] * inv), (__bf16)(o[4 * i + 1] * inv)};
        if (c + 2 < p.d) *reinterpret_cast<bf16x2*>(orow + 8 * i + 2) = (bf16x2){(__bf16)(o[4 * i + 2] * inv), (__bf16)(o[4 * i + 3] * inv)};
      }
    } else if (tvalid) {
      float* orow = p.out + (long long)mytok * p.ldo + p.o_off + g * p.d + 4 * hh;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 8 * i + 4 * hh;
        if (c < p.d) *reinterpret_cast<float2*>(orow + 8 * i) = (float2){o[4 * i] * inv, o[4 * i + 1] * inv};
        if (c + 2 < p.d) *reinterpret_cast<float2*>(orow + 8 * i + 2) = (float2){o[4 * i + 2] * inv, o[4 * i + 3] * inv};
      }
    }
    W2_STAMP(10 + 8 * hi);
  }
