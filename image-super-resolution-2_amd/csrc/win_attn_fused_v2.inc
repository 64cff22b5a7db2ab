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
  const FFWinId win = ff_win_decode(blockIdx.x, p.nwx, p.nwy);
  const int wx = win.wx, wy = win.wy, b = win.b;
  FF_STAMP(64, 0);

  // ---- LDS-DMA: a head's weight image (38 one-KiB pieces, 5 per wave) and its bias table (<= 10 pieces) ---------------------
#include "win_attn_fused_v2_dma.inc"
  dma_head(p.head0, 0);

  if (tid < 256) {
    const int qy = wy * WH + tid / WW, qx = wx * WW + tid % WW;
    ktok[tid] = ff_win_token(b, qy, qx, p.sh, p.sw, p.Hp, p.Wp, p.H, p.W);
    kreg[tid] = p.use_mask ? ff_win_region(qy, qx, p.Hp, p.Wp, WH, WW, p.sh, p.sw) : 0;
  }
  for (int i = tid; i < 3 * p.nheads * 32; i += 512) Bs[i] = p.bias ? p.bias[3 * p.head0 * 32 + i] : 0.f;
  __syncthreads();
  if (ONES && tid < p.nheads) Bs[(3 * tid + 2) * 32 + 30] = 1.0f;       // the denominator channel of V (visible after the first barrier below)

  const bool blk_mask = p.use_mask && ff_win_has_regions(wx, wy, p.nwx, p.nwy);
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
    // the gather below is win_attn_fused_kernel's with the read-back row reversed, written out in both: as a function and as one text
    // the assembly moved (see the note there)
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
#define W2_LN(f) p.f
#include "win_attn_fused_v2_ln.inc"
#undef W2_LN
  }
  FF_STAMP(64, 2);

#define W2_STAMP(i) FF_STAMP(64, i)
#include "win_attn_fused_v2_heads.inc"
#undef W2_STAMP
  FF_STAMP(64, 60);
  FF_STAMP_DRAINED(64, 61);
}
