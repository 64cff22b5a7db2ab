// HAT overlapping cross-attention (OCAB), attention stage, plain bf16:  16x16 query windows against 24x24 key windows
//   hat_arch.py:392-438 (OCAB.forward: unfold of k / v with kernel 24, stride 16, padding 4 -- zero keys outside the image --,
//   relative_position_bias_table[rpi_oca], softmax, attn @ v) -- the qkv projection before and the proj + MLP after are separate launches.
// One persistent workgroup per WINDOW walks the heads; what the two-stage kernel (attention_bf16.hip, one workgroup per window and
// head) paid for and this one does not:
//   * the bias came from an expanded [heads][576][256] table, 590 KB re-read from L2 per workgroup (3.3x the launch's algorithmic
//     traffic).  Here the head's compact 39 x 39 table sits in LDS, and the keys are walked in 4-row x 8-column tiles of the
//     24 x 24 window, so a lane's sixteen scores of a tile read at compile-time offsets from one base (row r>>2, column r&3 of the
//     tile): eight ds_read2_b32, no per-key offset table;
//   * K / V staging and attention ran back to back between two barriers per 128 keys.  Here a head's keys are two stages of nine
//     32-key tiles, double buffered: the rows of the next stage (or of the next head's first stage) are in flight in registers while
//     the current stage is computed -- one barrier per 288 keys;
//   * softmax as in win_attn_fused_v2: denominator through the padded V channel 30, running maximum exchanged with
//     v_permlane32_swap, rescale skipped while no maximum moves, output stored straight from the accumulators.
// The reference indexes its bias table with NEGATIVE numbers (offset a = ws - ows + 1 = -7) that PyTorch wraps; the table arrives
// rotated (prep.pack_rel_overlap) so that  i = 600 - 39 qy - qx + 39 ky + kx  is in [0, 1521).
// ROWS16 (ff_ocab_attn_rows16): q / k / v arrive as bf16 rows with every head slice padded from 30 to 32 channels (64 bytes, 16-byte
// aligned; channels 30 / 31 exact zeros, q already scaled) -- what ff_token_linear_rows16 writes from prep.pack_ocab_qkv's weights.  The
// fp32 form rounds the same values to bf16 as they arrive, so both forms feed the MFMAs the same operands; the rows form fetches them
// with 5 sixteen-byte loads per lane and stage instead of 18 eight-byte ones and converts nothing.
#include "ff_common.h"
#include "win_geometry.h"

#define OC_NK 576
#define OC_RELW 39
#define OC_RELN 1521
#define OC_STK 288                        // keys per stage: nine 32-key tiles = rows 12 s .. 12 s + 11 of the key window
#define OC_KROWB 80                       // K row: 32 bf16 + 16 B pad
#define OC_VROWB 592                      // V^T row: 288 bf16 + 16 B pad (148 dwords: conflict-free ds_read_b128 across channels)
#define OC_KBUF (OC_STK * OC_KROWB)
#define OC_VBUF (32 * OC_VROWB)
#define OC_STAGEB (OC_KBUF + OC_VBUF)
#define OC_OFF_REL (2 * OC_STAGEB)
#define OC_RELB (1536 * 4)
#define OC_OFF_TOK (OC_OFF_REL + 2 * OC_RELB)
#define OC_LDS (OC_OFF_TOK + OC_NK * 4)
#define OC_NLOAD 18                       // 288 keys / 16 keys per pass
#define OC_NLOAD16 5                      // ROWS16: 288 keys x 8 sixteen-byte quarters (4 of k, 4 of v) / 512 lanes, last pass half-masked

struct OcabParams {
  const float* qkv; float* out; const float* rel;
  int ldq, ldo, q_off, k_off, v_off, o_off, B, H, W, nwx, nwy, heads, out_bf16;
  float scale;
  FF_STAMP_MEMBER
};

template <bool ROWS16>
__global__ __launch_bounds__(512) void ocab_attn_kernel(OcabParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* ktok = reinterpret_cast<int*>(smem + OC_OFF_TOK);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, hh = lane >> 5;
  const FFWinId win = ff_win_decode(blockIdx.x, p.nwx, p.nwy);
  const int wx = win.wx, wy = win.wy, b = win.b;
  FF_STAMP(64, 0);

  // ---- key table in TILE order: key index 32 T + kappa, T = 3 tr + tc, is window position (4 tr + kappa / 8, 8 tc + kappa % 8) ---
  for (int kidx = tid; kidx < OC_NK; kidx += 512) {
    const int T = kidx >> 5, kap = kidx & 31;
    const int ky = 4 * (T / 3) + (kap >> 3), kx = 8 * (T % 3) + (kap & 7);
    const int y = wy * 16 - 4 + ky, x = wx * 16 - 4 + kx;
    ktok[kidx] = FF_WIN_IN_IMAGE(y, x, p.H, p.W) ? (b * p.H + y) * p.W + x : -1;      // (the text form: a token function moved the assembly)
  }
  // constant parts of both stage buffers: K channels 30 / 31 = 0, V^T row 30 = 1 (the denominator channel), row 31 = 0
  for (int i = tid; i < 2 * OC_STK; i += 512)
    *reinterpret_cast<unsigned*>(smem + (i / OC_STK) * OC_STAGEB + (i % OC_STK) * OC_KROWB + 60) = 0u;
  for (int i = tid; i < 2 * 2 * (OC_VROWB / 4); i += 512) {
    const int buf = i / (2 * (OC_VROWB / 4)), r = i % (2 * (OC_VROWB / 4));
    const int row = 30 + r / (OC_VROWB / 4), col = r % (OC_VROWB / 4);
    *reinterpret_cast<unsigned*>(smem + buf * OC_STAGEB + OC_KBUF + row * OC_VROWB + 4 * col) = row == 30 ? 0x3F803F80u : 0u;
  }
  __syncthreads();

  const int qi = wid * 32 + l31;
  const int qy = qi >> 4, qx = qi & 15;
  const int ty = wy * 16 + qy, tx = wx * 16 + qx;
  const bool qvalid = ty < p.H && tx < p.W;
  const long long qtok = qvalid ? (long long)(b * p.H + ty) * p.W + tx : 0;
  const int rel_lane = 600 - OC_RELW * qy - qx + 4 * hh;
  const float LOG2E = 1.4426950408889634f;

  // ---- staging: lane & 31 = float2 pair of a key's head slice (0..14 k, 15..29 v, 30 / 31 idle), (tid >> 5) + 16 i = key of the stage:
  //      no per-element index arithmetic, a wave instruction fetches the four 120-byte k / v segments of two keys --------------------
  const int spr = tid & 31, skey = tid >> 5;
  const bool s_on = spr < 30, s_isk = spr < 15;
  const int s_ch = s_isk ? p.k_off + 2 * spr : p.v_off + 2 * (spr - 15);
  float2 stg[ROWS16 ? 1 : OC_NLOAD];
  float tb[3];
  float2 qn[ROWS16 ? 1 : 8];
  // ROWS16 staging: item = tid + 512 i of the stage is quarter (item & 7) of key (item >> 3): quarters 0..3 are the key's k slice,
  // 4..7 its v slice, so eight neighbouring lanes fetch the two 64-byte segments of one key
  const __bf16* qkv16 = reinterpret_cast<const __bf16*>(p.qkv);
  const int s_qt = tid & 7;
  const int s_ch16 = s_qt < 4 ? p.k_off + 8 * s_qt : p.v_off + 8 * (s_qt - 4);
  bf16x8 stg16[ROWS16 ? OC_NLOAD16 : 1];
  bf16x8 qn16[2];
  unsigned stg_ok = 0u;                                 // validity of the staged keys (bit i): applied when the stage is STORED -- a select
                                                        // on the loaded value here would make every load wait for its data (measured: 3.5 us
                                                        // per stage just to "issue" the loads, tools/oc_time.cpp)
  // in two halves: a wave stalls at issue once it has more than a dozen or so loads outstanding (tools/oc_time.cpp: "issuing" all 18 took
  // 3.6 us = the latency of the first ones); the second half is issued a third of the way into the stage's tiles
  auto stage_load = [&](int h, int st, int part) {
    if constexpr (ROWS16) {                             // five loads: all of them at the start of the stage
      if (part == 0) {
        stg_ok = 0u;
#pragma unroll
        for (int i = 0; i < OC_NLOAD16; ++i) {
          const int kl = (tid + 512 * i) >> 3;
          const int tk = kl < OC_STK ? ktok[st * OC_STK + kl] : -1;
          stg_ok |= (tk >= 0 ? 1u : 0u) << i;
          stg16[i] = *reinterpret_cast<const bf16x8*>(qkv16 + (tk >= 0 ? (long long)tk * p.ldq : 0) + s_ch16 + h * 32);
        }
      }
    } else {
      if (part == 0) stg_ok = 0u;
#pragma unroll
      for (int i = 0; i < OC_NLOAD; ++i) {
        if ((i < OC_NLOAD / 2) != (part == 0)) continue;
        const int tk = s_on ? ktok[st * OC_STK + skey + 16 * i] : -1;
        stg_ok |= (tk >= 0 ? 1u : 0u) << i;
        stg[i] = *reinterpret_cast<const float2*>(p.qkv + (tk >= 0 ? (long long)tk * p.ldq + s_ch + h * 30 : 0));
      }
    }
  };
  auto stage_store = [&](int buf) {
    unsigned char* kb = smem + buf * OC_STAGEB;
    unsigned char* vb = kb + OC_KBUF;
    if constexpr (ROWS16) {
#pragma unroll
      for (int i = 0; i < OC_NLOAD16; ++i) {
        const int kl = (tid + 512 * i) >> 3;
        if (kl >= OC_STK) continue;                       // second half of the last pass
        const bool ok = (stg_ok >> i) & 1u;
        const bf16x8 z = {};
        const bf16x8 val = ok ? stg16[i] : z;
        if (s_qt < 4) {
          *reinterpret_cast<bf16x8*>(kb + kl * OC_KROWB + 16 * s_qt) = val;
        } else {
          const int ch = 8 * (s_qt - 4), pos = ff_swap23(kl);
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (e < 6 || s_qt < 7) *reinterpret_cast<__bf16*>(vb + (ch + e) * OC_VROWB + 2 * pos) = val[e];    // rows 30 / 31 are the kernel's constants
        }
      }
    } else if (s_on) {
#pragma unroll
      for (int i = 0; i < OC_NLOAD; ++i) {
        const int kl = skey + 16 * i;
        const bool ok = (stg_ok >> i) & 1u;
        const __bf16 a = (__bf16)(ok ? stg[i].x : 0.f), c = (__bf16)(ok ? stg[i].y : 0.f);
        if (s_isk) {
          const unsigned pk = (unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, c) << 16);
          *reinterpret_cast<unsigned*>(kb + kl * OC_KROWB + 4 * spr) = pk;
        } else {
          const int ch = 2 * (spr - 15), pos = ff_swap23(kl);
          *reinterpret_cast<__bf16*>(vb + ch * OC_VROWB + 2 * pos) = a;
          *reinterpret_cast<__bf16*>(vb + (ch + 1) * OC_VROWB + 2 * pos) = c;
        }
      }
    }
  };
  auto head_load = [&](int h) {                        // bias table and queries of head h
#pragma unroll
    for (int i = 0; i < 3; ++i) tb[i] = (tid + 512 * i < OC_RELN) ? p.rel[(long long)h * OC_RELN + tid + 512 * i] : 0.f;
    if constexpr (ROWS16) {                             // channels 16 s + 8 hh .. + 7 of the head's 32-wide slice: the MFMA operand as stored
#pragma unroll
      for (int s = 0; s < 2; ++s) qn16[s] = *reinterpret_cast<const bf16x8*>(qkv16 + qtok * p.ldq + p.q_off + h * 32 + 16 * s + 8 * hh);
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int dd = 16 * s + 8 * hh + 2 * j;
          qn[4 * s + j] = dd < 30 ? *reinterpret_cast<const float2*>(p.qkv + qtok * p.ldq + p.q_off + h * 30 + dd) : (float2){0.f, 0.f};
        }
    }
  };
  bf16x8 qh[2];
  auto head_store = [&](int h) {
    float* tl = reinterpret_cast<float*>(smem + OC_OFF_REL + (h & 1) * OC_RELB);
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (tid + 512 * i < OC_RELN) tl[tid + 512 * i] = tb[i];
    if constexpr (ROWS16) {
      const bf16x8 z = {};
#pragma unroll
      for (int s = 0; s < 2; ++s) qh[s] = qvalid ? qn16[s] : z;
    } else {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool ok = qvalid;
          qh[s][2 * j] = (__bf16)(ok ? qn[4 * s + j].x * p.scale : 0.f);
          qh[s][2 * j + 1] = (__bf16)(ok ? qn[4 * s + j].y * p.scale : 0.f);
        }
    }
  };

  stage_load(0, 0, 0);
  stage_load(0, 0, 1);
  head_load(0);
  stage_store(0);
  head_store(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  FF_STAMP(64, 1);
  f32x16 o;
  float m_run = -INFINITY;
  const int nsteps = 2 * p.heads;
  for (int n = 0; n < nsteps; ++n) {
    const int h = n >> 1, st = n & 1, buf = n & 1;
    const bool more = n + 1 < nsteps;
    if (more) {
      stage_load((n + 1) >> 1, (n + 1) & 1, 0);
      if (st == 1) head_load(h + 1);
    }
    if (n < 4) FF_STAMP(64, 2 + 4 * n);
    if (st == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = 0.f;
      m_run = -INFINITY;
    }
    const unsigned char* kb = smem + buf * OC_STAGEB + l31 * OC_KROWB + 16 * hh;
    const unsigned char* vb = smem + buf * OC_STAGEB + OC_KBUF + l31 * OC_VROWB + 16 * hh;
    const unsigned rel0 = (unsigned)(size_t)(__attribute__((address_space(3))) const void*)(smem + OC_OFF_REL + (h & 1) * OC_RELB) +
                          4u * (unsigned)(rel_lane + st * (12 * OC_RELW));
    for (int tq = 0; tq < 3; ++tq) {
      if (more && tq == 1) stage_load((n + 1) >> 1, (n + 1) & 1, 1);
#pragma unroll
      for (int tm = 0; tm < 3; ++tm) {
        const int t = 3 * tq + tm;
        unsigned ra = rel0 + 4u * (unsigned)(tq * 4 * OC_RELW + tm * 8);
        asm volatile("" : "+v"(ra));                    // one base register per tile: the gathers below use immediate offsets
        const ff_lds_cf relp = (ff_lds_cf)(size_t)ra;
        f32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = relp[(r >> 2) * OC_RELW + (r & 3)];
        bf16x8 vh2[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) vh2[s] = *reinterpret_cast<const bf16x8*>(vb + t * 64 + 32 * s);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8 ah = *reinterpret_cast<const bf16x8*>(kb + t * 32 * OC_KROWB + 32 * s);
          sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, qh[s], sc, 0, 0, 0);
        }
        float mx = sc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sc[r]);
        {
          float lo, hi;
          ff_halves(mx, lo, hi);
          mx = fmaxf(lo, hi);
        }
        if (__builtin_amdgcn_ballot_w64(mx > m_run) != 0) {
          const float m_new = fmaxf(m_run, mx);
          const float corr = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
#pragma unroll
          for (int r = 0; r < 16; ++r) o[r] *= corr;
          m_run = m_new;
        }
        const float mneg = -m_run * LOG2E;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8 ph;
#pragma unroll
          for (int j = 0; j < 8; ++j) ph[j] = (__bf16)__builtin_amdgcn_exp2f(__builtin_fmaf(sc[8 * s + j], LOG2E, mneg));
          o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh2[s], ph, o, 0, 0, 0);
        }
      }
    }
    if (n < 4) FF_STAMP(64, 3 + 4 * n);
    if (st == 1) {                                       // head finished: channel 30 = register 14 of the upper half-wave holds sum(P)
      float lo, den;
      ff_halves(o[14], lo, den);
      const float inv = 1.0f / den;
      if (qvalid && p.out_bf16) {                       // bf16 rows (ldo in elements): the consumer rounds to bf16 anyway
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        __bf16* orow = reinterpret_cast<__bf16*>(p.out) + qtok * p.ldo + p.o_off + h * 30 + 4 * hh;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = 8 * i + 4 * hh;
          if (c < 30) *reinterpret_cast<bf16x2*>(orow + 8 * i) = (bf16x2){(__bf16)(o[4 * i] * inv), (__bf16)(o[4 * i + 1] * inv)};
          if (c + 2 < 30) *reinterpret_cast<bf16x2*>(orow + 8 * i + 2) = (bf16x2){(__bf16)(o[4 * i + 2] * inv), (__bf16)(o[4 * i + 3] * inv)};
        }
      } else if (qvalid) {
        float* orow = p.out + qtok * p.ldo + p.o_off + h * 30 + 4 * hh;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = 8 * i + 4 * hh;
          if (c < 30) *reinterpret_cast<float2*>(orow + 8 * i) = (float2){o[4 * i] * inv, o[4 * i + 1] * inv};
          if (c + 2 < 30) *reinterpret_cast<float2*>(orow + 8 * i + 2) = (float2){o[4 * i + 2] * inv, o[4 * i + 3] * inv};
        }
      }
    }
    if (more) {
      stage_store(buf ^ 1);
      if (st == 1) head_store(h + 1);
    }
    if (n < 4) FF_STAMP(64, 4 + 4 * n);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                        // the next stage is in LDS; every wave is done with this one
    if (n < 4) FF_STAMP(64, 5 + 4 * n);
  }
  FF_STAMP(64, 60);
}

template <bool ROWS16>
static int ocab_launch(OcabParams& p, const char* who, void* stream) {
  FF_STAMP_ARM(p);
  const long long nblk = (long long)p.B * p.nwx * p.nwy;
  FF_CHECK_ARG(nblk < (1LL << 31), "%s: grid too large", who);
  static_assert(OC_LDS <= FF_LDS_MAX, "LDS image too large");
  static ff_device_once once;
  if (!ff_raise_lds(once, who, OC_LDS, FF_LDS_SAY_ERR, &ocab_attn_kernel<ROWS16>)) return FF_ERR_LAUNCH;
  hipLaunchKernelGGL(ocab_attn_kernel<ROWS16>, dim3((unsigned)nblk), dim3(512), OC_LDS, (hipStream_t)stream, p);
  FF_LAUNCH_CHECK(who);
  return FF_OK;
}

extern "C" int ff_ocab_attn(const float* qkv, int ldq, int q_off, int k_off, int v_off, float* out, int ldo, int o_off,
                            const float* rel_rotated, int B, int H, int W, int heads, int d, int ws, int ows, float scale, int out_bf16, void* stream) {
  FF_CHECK_ARG(qkv && out && rel_rotated, "ff_ocab_attn: null pointer");
  FF_CHECK_ARG(ws == 16 && ows == 24 && d == 30 && heads > 0, "ff_ocab_attn: built for 16x16 query / 24x24 key windows and head dim 30 (got %d / %d / %d)", ws, ows, d);
  FF_CHECK_ARG(B > 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "ff_ocab_attn: H and W must be multiples of the window");
  FF_CHECK_ARG(ldq % 2 == 0 && q_off % 2 == 0 && k_off % 2 == 0 && v_off % 2 == 0 && (((uintptr_t)qkv) & 7) == 0, "ff_ocab_attn: qkv rows must be 8-byte aligned");
  FF_CHECK_ARG(ldo % 2 == 0 && o_off % 2 == 0 && (((uintptr_t)out) & 7) == 0 && ldo >= o_off + heads * d, "ff_ocab_attn: out rows must be 8-byte aligned and hold every head");
  FF_CHECK_ARG((long long)B * H * W * (ldq > ldo ? ldq : ldo) < (1LL << 31), "ff_ocab_attn: tensor too large for 32-bit token offsets");
  OcabParams p;
  p.qkv = qkv; p.out = out; p.rel = rel_rotated; p.ldq = ldq; p.ldo = ldo; p.q_off = q_off; p.k_off = k_off; p.v_off = v_off; p.o_off = o_off;
  p.B = B; p.H = H; p.W = W; p.nwx = W / 16; p.nwy = H / 16; p.heads = heads; p.scale = scale; p.out_bf16 = out_bf16;
  return ocab_launch<false>(p, "ff_ocab_attn", stream);
}

// The rows form: qkv16 holds bf16 rows [B*H*W][ldq] (ldq in elements) with head h of q / k / v at q_off / k_off / v_off + 32 h: 30
// channels and two exact zeros, q already multiplied by the softmax scale.  Base and pitch are 16-byte aligned, the offsets multiples of 32.
extern "C" int ff_ocab_attn_rows16(const void* qkv16, int ldq, int q_off, int k_off, int v_off, float* out, int ldo, int o_off,
                                   const float* rel_rotated, int B, int H, int W, int heads, int d, int ws, int ows, int out_bf16, void* stream) {
  FF_CHECK_ARG(qkv16 && out && rel_rotated, "ff_ocab_attn_rows16: null pointer");
  FF_CHECK_ARG(ws == 16 && ows == 24 && d == 30 && heads > 0, "ff_ocab_attn_rows16: built for 16x16 query / 24x24 key windows and head dim 30 (got %d / %d / %d)", ws, ows, d);
  FF_CHECK_ARG(B > 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, "ff_ocab_attn_rows16: H and W must be multiples of the window");
  FF_CHECK_ARG(ldq > 0 && ldq % 8 == 0 && (((uintptr_t)qkv16) & 15) == 0, "ff_ocab_attn_rows16: qkv rows must be 16-byte aligned (pitch %d in bf16 elements)", ldq);
  FF_CHECK_ARG(q_off >= 0 && k_off >= 0 && v_off >= 0 && q_off % 32 == 0 && k_off % 32 == 0 && v_off % 32 == 0, "ff_ocab_attn_rows16: q / k / v offsets must be multiples of 32 (got %d / %d / %d)", q_off, k_off, v_off);
  FF_CHECK_ARG(ldq >= q_off + heads * 32 && ldq >= k_off + heads * 32 && ldq >= v_off + heads * 32, "ff_ocab_attn_rows16: rows too short for %d padded heads", heads);
  FF_CHECK_ARG(ldo % 2 == 0 && o_off % 2 == 0 && o_off >= 0 && (((uintptr_t)out) & 7) == 0 && ldo >= o_off + heads * d, "ff_ocab_attn_rows16: out rows must be 8-byte aligned and hold every head");
  FF_CHECK_ARG((long long)B * H * W * (ldq > ldo ? ldq : ldo) < (1LL << 31), "ff_ocab_attn_rows16: tensor too large for 32-bit token offsets");
  OcabParams p;
  p.qkv = reinterpret_cast<const float*>(qkv16); p.out = out; p.rel = rel_rotated; p.ldq = ldq; p.ldo = ldo; p.q_off = q_off; p.k_off = k_off; p.v_off = v_off; p.o_off = o_off;
  p.B = B; p.H = H; p.W = W; p.nwx = W / 16; p.nwy = H / 16; p.heads = heads; p.scale = 1.0f; p.out_bf16 = out_bf16;
  return ocab_launch<true>(p, "ff_ocab_attn_rows16", stream);
}
