// Plain-bf16 form of the window-resident attention block (included by win_attn_fused.hip; same parameters, same outputs).
// What differs from the split-bf16 kernel above, all of it scheduling:
//   * the three weight tiles of a head are ONE LDS image, fetched by LDS-DMA while the previous head's attention runs;
//     K, V^T and the bias table are double buffered, so a head costs two workgroup barriers instead of five and no wave
//     waits on HBM (the measured head-to-head transition of the ring form was 2.3 us of 11.2 us per head);
//   * lane l of a wave holds window position 32 w + 31 - l: with keys DESCENDING in the accumulator registers the bias
//     gather runs over ascending addresses (ds_read2 pairs land in place: 16 register moves per tile gone);
//   * head dim 30: padded V channel 30 is the constant 1 (bias 1, zero weights), so the PV MFMA accumulates the softmax
//     denominator in accumulator register 14 of the upper half-wave -- 16 adds per tile gone;
//   * the running maximum is exchanged with v_permlane32_swap (no LDS round trip) and the O / denominator rescale is skipped
//     while no lane's maximum moves;
//   * head dim 30: the shift mask rides in the two padded q/k channels (q30 k30 + q31 k31 = +-50 +-50: keys of another
//     region score 100 or 200 lower, which is the reference's -100 to within e^-100) -- no per-tile mask arithmetic;
//   * O^T is stored straight from the accumulators (lane = token): no LDS transpose, no wait.
#define W2_TILEB (32 * WF_ROWB)                       // one 32-row weight tile, hi plane: 12 800 B
#define W2_HEAD_SLOTS (3 * WF_PL)                     // 16-byte slots of a head's q|k|v image
#define W2_PIECES ((W2_HEAD_SLOTS + 63) / 64)         // 1-KiB DMA pieces (38)
#define W2_WB (W2_PIECES * 1024)
#define W2_KROWB 80
#define W2_KWAVE (32 * W2_KROWB)
#define W2_KBUF (8 * W2_KWAVE)
#define W2_VROWB 528
#define W2_VBUF (32 * W2_VROWB)
#define W2_RELB ((WF_REL_MAX + WF_REL_PAD) * 4)
#define W2_OFF_K W2_WB
#define W2_OFF_V (W2_OFF_K + 2 * W2_KBUF)
#define W2_OFF_REL (W2_OFF_V + 2 * W2_VBUF)
#define W2_OFF_BS (W2_OFF_REL + 2 * W2_RELB)
#define W2_OFF_TOK (W2_OFF_BS + WF_BS_MAX * 4)
#define W2_OFF_REG (W2_OFF_TOK + 1024)
#define W2_OFF_SAME (W2_OFF_REG + 1024)
#define W2_LDS (W2_OFF_SAME + 9 * 8 * 4)

template <int WW, bool ONES>
__global__ __launch_bounds__(512) void win_attn_fused_v2_kernel(WinFusedParams p) {
  constexpr int WH = 256 / WW;
  constexpr int RS = WW == 8 ? 40 : (WW == 16 ? 48 : 64);
  constexpr int TPR = WW >= 32 ? 1 : 32 / WW;          // key rows of the window per 32-key tile
  constexpr int WWM = WW >= 32 ? 32 : WW;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* Bs = reinterpret_cast<float*>(smem + W2_OFF_BS);
  int* ktok = reinterpret_cast<int*>(smem + W2_OFF_TOK);
  int* kreg = reinterpret_cast<int*>(smem + W2_OFF_REG);
  unsigned* same = reinterpret_cast<unsigned*>(smem + W2_OFF_SAME);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  int bid = blockIdx.x;
  const int wx = bid % p.nwx; bid /= p.nwx;
  const int wy = bid % p.nwy;
  const int b = bid / p.nwy;
  FF_STAMP(64, 0);

  // ---- LDS-DMA: a head's weight image (38 one-KiB pieces, 5 per wave) and its bias table (<= 10 pieces) ---------------------
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
  dma_head(p.head0, 0);

  if (tid < 256) {
    const int qy = wy * WH + tid / WW, qx = wx * WW + tid % WW;
    int oy = qy + p.sh, ox = qx + p.sw;
    if (oy >= p.Hp) oy -= p.Hp;
    if (ox >= p.Wp) ox -= p.Wp;
    ktok[tid] = (oy < p.H && ox < p.W) ? (b * p.H + oy) * p.W + ox : -1;
    int rid = 0;
    if (p.use_mask) {
      const int ry = qy < p.Hp - WH ? 0 : (qy < p.Hp - p.sh ? 1 : 2);
      const int rx = qx < p.Wp - WW ? 0 : (qx < p.Wp - p.sw ? 1 : 2);
      rid = 3 * ry + rx;
    }
    kreg[tid] = rid;
  }
  for (int i = tid; i < 3 * p.nheads * 32; i += 512) Bs[i] = p.bias ? p.bias[3 * p.head0 * 32 + i] : 0.f;
  __syncthreads();
  if (ONES && tid < p.nheads) Bs[(3 * tid + 2) * 32 + 30] = 1.0f;       // the denominator channel of V (visible after the first barrier below)

  const bool blk_mask = p.use_mask && (wy == p.nwy - 1 || wx == p.nwx - 1);
  if (!ONES && blk_mask) {                             // key-region bit masks, bit i of tile t = key 32 t + 31 - i
    for (int i = wid; i < 72; i += 8) {
      const int region = i >> 3, t = i & 7;
      const unsigned long long bal = __ballot(l31 == lane && kreg[32 * t + 31 - l31] == region);
      if (lane == 0) same[i] = (unsigned)bal;
    }
    __syncthreads();
  }
  const int qi = wid * 32 + 31 - l31;                  // this lane's window position (query; also one of the wave's keys)
  const int mytok = ktok[qi];
  const bool tvalid = mytok >= 0;
  const int qreg_id = kreg[qi];
  const unsigned vmask = (unsigned)(__ballot(tvalid) & 0xffffffffu);
  const bool kill_pad = p.zero_pad != 0;
  // shift mask as two extra q/k channels: +-7.0625 (bf16-exact, square 49.88) by the token's row / column region
  const float msy = (qreg_id / 3 == 2) ? -7.0625f : 7.0625f, msx = (qreg_id % 3 == 2) ? -7.0625f : 7.0625f;
  FF_STAMP(64, 1);

  // ---- the wave's 32 rows of x -> LayerNorm -> bf16 fragments -----------------------------------------------------------------
  bf16x8 xh[WF_KS];
  {
    float* xs = reinterpret_cast<float*>(smem + W2_OFF_K) + wid * (32 * WF_XS_ROW);    // gather patch over the idle K/V area
    const int rr = lane >> 4, cq = (lane & 15) * 4;
    float v[WF_KS][8];
    f32x4 t[3][8];
#pragma unroll
    for (int pass = 0; pass < 3; ++pass)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = 4 * j + rr, c = 64 * pass + cq;
        const int tk = ktok[wid * 32 + r];
        const bool ok = tk >= 0 && c < p.K;
        const f32x4 u = *reinterpret_cast<const f32x4*>(p.x + (ok ? (long long)tk * p.ldx + c : 0));
        t[pass][j] = ok ? u : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    const float* xrow = xs + (31 - l31) * WF_XS_ROW + 8 * hh;
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
#pragma unroll
      for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(xs + (4 * j + rr) * WF_XS_ROW + cq) = t[pass][j];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(xrow + 16 * s4);
        const f32x4 c4 = *reinterpret_cast<const f32x4*>(xrow + 16 * s4 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[4 * pass + s4][e] = a[e]; v[4 * pass + s4][4 + e] = c4[e]; }
      }
    }
    // every load of this wave has returned (the x rows were consumed above; the head-0 DMA left long before them): the
    // side-output stores below are then the only traffic in flight and nothing later has to wait for them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ff_frag_ln_stats, inline on purpose: with the helper every instantiation goes from 171 / 196 to 246 VGPRs and
    // win_attn_fused_v2_kernel<32, true> from 46.17 / 45.91 us to 46.36 / 47.23 us under the bench
    float mean = 0.f, rstd = 1.f;
    if (p.gamma) {
      float s = 0.f;
#pragma unroll
      for (int st = 0; st < WF_KS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[st][j];
      s += __shfl_xor(s, 32);
      mean = s / (float)p.K;
      float qv = 0.f;
#pragma unroll
      for (int st = 0; st < WF_KS; ++st)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float dd = (16 * st + 8 * hh + j < p.K) ? v[st][j] - mean : 0.f;
          qv += dd * dd;
        }
      qv += __shfl_xor(qv, 32);
      rstd = 1.0f / sqrtf(qv / (float)p.K + p.eps);
    }
#pragma unroll
    for (int st = 0; st < WF_KS; ++st) {
      const int k0 = 16 * st + 8 * hh;
      f32x4 g0 = {1.f, 1.f, 1.f, 1.f}, g1 = g0, b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
      if (p.gamma) {
        const int ka = k0 < p.K ? k0 : 0, kb = k0 + 4 < p.K ? k0 + 4 : 0;
        g0 = *reinterpret_cast<const f32x4*>(p.gamma + ka); b0 = *reinterpret_cast<const f32x4*>(p.beta + ka);
        g1 = *reinterpret_cast<const f32x4*>(p.gamma + kb); b1 = *reinterpret_cast<const f32x4*>(p.beta + kb);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float gg = j < 4 ? g0[j & 3] : g1[j & 3], bb = j < 4 ? b0[j & 3] : b1[j & 3];
        const float f = (k0 + j < p.K) ? (p.gamma ? (v[st][j] - mean) * rstd * gg + bb : v[st][j]) : 0.f;
        xh[st][j] = (__bf16)f;
        v[st][j] = f;
      }
      if (p.xn && tvalid && p.xn_bf16) {             // bf16 side output: the fragment itself (its consumer rounds to bf16 anyway)
        if (k0 < p.K) *reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(p.xn) + (long long)mytok * p.ldxn + k0) = xh[st];
      } else if (p.xn && tvalid) {
        float* xr = p.xn + (long long)mytok * p.ldxn + k0;
        if (k0 < p.K) *reinterpret_cast<f32x4*>(xr) = (f32x4){v[st][0], v[st][1], v[st][2], v[st][3]};
        if (k0 + 4 < p.K) *reinterpret_cast<f32x4*>(xr + 4) = (f32x4){v[st][4], v[st][5], v[st][6], v[st][7]};
      }
    }
  }
  FF_STAMP(64, 2);

  // bias[q][k] = T[(qy - ky + WH-1) RS + (qx - kx + WW-1)].  Register r of a lane holds key 32 t + 31 - c of tile t,
  // c = (r & 3) + 8 (r >> 2) + 4 hh, so the index is (lane part) - (tile part) + (c / WW) RS + (c % WW): ascending in r
  const int rel_lane = ((qi / WW) + WH - 1) * RS + (qi % WW) + WW - 1 - (TPR - 1) * RS - (WWM - 1) + 4 * hh;
  const float LOG2E = 1.4426950408889634f;

  auto gemm_tile = [&](int j, bool swap, f32x16& acc) {
    const unsigned char* ap = smem + j * W2_TILEB + l31 * WF_ROWB + 16 * hh;
    bf16x8 fa[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) fa[u] = *reinterpret_cast<const bf16x8*>(ap + 32 * u);
#pragma unroll
    for (int st = 0; st < WF_KS; ++st) {
      const bf16x8 ah = fa[st & 1];
      if (st + 2 < WF_KS) fa[st & 1] = *reinterpret_cast<const bf16x8*>(ap + 32 * (st + 2));
      __builtin_amdgcn_sched_barrier(0);
      if (!swap) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xh[st], acc, 0, 0, 0);
      else acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[st], ah, acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  for (int hi = 0; hi < p.nheads; ++hi) {
    const int g = p.head0 + hi, buf = hi & 1;
    unsigned char* KB = smem + W2_OFF_K + buf * W2_KBUF;
    unsigned char* VB = smem + W2_OFF_V + buf * W2_VBUF;
    // every wave has confirmed its DMA pieces of this head (vmcnt(0) above / at the end of the previous attention) and is
    // past the previous head's attention
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    FF_STAMP(64, 3 + 8 * hi);
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
    FF_STAMP(64, 4 + 8 * hi);
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
    FF_STAMP(64, 5 + 8 * hi);
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
    FF_STAMP(64, 6 + 8 * hi);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                       // K and V^T of this head are complete; every wave is done with the weight image
    FF_STAMP(64, 7 + 8 * hi);
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
    FF_STAMP(64, 8 + 8 * hi);
    // the next head's DMA (issued ~an attention ago) and the side-output stores have landed: confirmed here, BEFORE this
    // head's output stores enter the queue, so that no later wait has to drain them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FF_STAMP(64, 9 + 8 * hi);

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
    FF_STAMP(64, 10 + 8 * hi);
  }
  FF_STAMP(64, 60);
  FF_STAMP_DRAINED(64, 61);
}
