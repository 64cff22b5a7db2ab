// Shared helpers for the FreqFusion HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "ff_device_once.h"
#include "lds_layout.h"       // the older kernels' LDS maps (host + device; token_mlp_layout.h and win_attn_layout.h hold the newer ones)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const float* ff_lds_cf;

#define FF_OK 0
#define FF_ERR_ARG 1
#define FF_ERR_LAUNCH 2

extern "C" const char* ff_last_error(void);
void ff_set_error(const char* fmt, ...);

#define FF_CHECK_ARG(cond, ...)          \
  do {                                   \
    if (!(cond)) {                       \
      ff_set_error(__VA_ARGS__);         \
      return FF_ERR_ARG;                 \
    }                                    \
  } while (0)

#define FF_LAUNCH_CHECK(name)                                              \
  do {                                                                     \
    hipError_t e__ = hipGetLastError();                                    \
    if (e__ != hipSuccess) {                                               \
      ff_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
      return FF_ERR_LAUNCH;                                                \
    }                                                                      \
  } while (0)

// what a workgroup can ask for on gfx950, and what it gets without hipFuncAttributeMaxDynamicSharedMemorySize
#define FF_LDS_MAX (160 * 1024)
#define FF_LDS_DEFAULT_MAX (64 * 1024)

// ---- dynamic LDS above the 64 KB default ----------------------------------------------------------------------------------------
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to a (kernel, device) pair.  A launch site keeps one `static ff_device_once` -- one
// per instantiation where the site is a template or a launch macro -- and raises its kernel(s) through it before the launch: once per
// device, from any thread (two first callers may both set the attribute, which is harmless).  On failure the error text is
// "<who>: cannot raise dynamic LDS[ to <bytes>][: <hip error>]", `say` picking the parts (every entry point keeps the wording it always
// had), and the site returns FF_ERR_LAUNCH.
enum { FF_LDS_SAY_ERR = 1, FF_LDS_SAY_SIZE = 2 };
template <class... Kernel>
static inline bool ff_raise_lds(ff_device_once& once, const char* who, size_t bytes, int say, Kernel*... kernels) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) { ff_set_error("%s: cannot identify the device: %s", who, hipGetErrorString(e)); return false; }
  return once.run(dev, [&] {
    ((e = e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void*>(kernels), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)), ...);
    if (e == hipSuccess) return true;
    char to[32] = "";
    if (say & FF_LDS_SAY_SIZE) snprintf(to, sizeof to, " to %zu", bytes);
    ff_set_error("%s: cannot raise dynamic LDS%s%s%s", who, to, (say & FF_LDS_SAY_ERR) ? ": " : "", (say & FF_LDS_SAY_ERR) ? hipGetErrorString(e) : "");
    return false;
  });
}

// ---- phase stamps: a debug aid of tools/*_time.cpp, compiled in with -DFF_TIMING only -------------------------------------------
// A kernel's params struct carries FF_STAMP_MEMBER, its entry point says FF_STAMP_ARM(p), and lane 0 of every wave writes
// wall_clock64() (100 MHz) into slot i of its row of the stamp buffer [block][8 waves][per_wave] with FF_STAMP(per_wave, i);
// FF_STAMP_DRAINED waits for the wave's outstanding stores first.  Without FF_TIMING the member expands to nothing and the others to an empty statement.
#ifdef FF_TIMING
static unsigned long long* g_ff_stamps = nullptr;      // set by the tool; nullptr = no stamps
#define FF_STAMP_MEMBER unsigned long long* dbg;
#define FF_STAMP_ARM(p) (p).dbg = g_ff_stamps
#define FF_STAMP(per_wave, i)                                                                                             \
  do {                                                                                                                    \
    if (p.dbg && (threadIdx.x & 63) == 0)                                                                                 \
      p.dbg[((long long)blockIdx.x * 8 + (threadIdx.x >> 6)) * (per_wave) + (i)] = wall_clock64();                        \
  } while (0)
#define FF_STAMP_DRAINED(per_wave, i)                    \
  do {                                                   \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     \
    FF_STAMP(per_wave, i);                               \
  } while (0)
#else
#define FF_STAMP_MEMBER
#define FF_STAMP_ARM(p) do { } while (0)
#define FF_STAMP(per_wave, i) do { } while (0)               // (a statement: `if (ht < 3) FF_STAMP(..);` stays well formed)
#define FF_STAMP_DRAINED(per_wave, i) do { } while (0)
#endif

// activation codes shared by every epilogue (include/ff_kernels.h FF_ACT_*)
enum { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2, ACT_LRELU = 3, ACT_SIGMOID = 4 };

__device__ __forceinline__ float ff_act(float v, int act) {
  switch (act) {
    case ACT_GELU: return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    case ACT_RELU: return v > 0.f ? v : 0.f;
    case ACT_LRELU: return v > 0.f ? v : 0.01f * v;
    case ACT_SIGMOID: return 1.0f / (1.0f + expf(-v));
    default: return v;
  }
}

// GELU with the Abramowitz-Stegun 7.1.26 erf (|error| <= 1.5e-7): ~14 VALU ops instead of ~55 for libm erff with its
// two divergent branches.  Used by the split-bf16 kernels (whose own error is ~1e-5); the f32 parity kernels keep erff.
__device__ __forceinline__ float ff_gelu_fast(float v) {
  const float ax = fabsf(v) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, ax, 1.0f));
  float pl = __builtin_fmaf(1.061405429f, t, -1.453152027f);
  pl = __builtin_fmaf(pl, t, 1.421413741f);
  pl = __builtin_fmaf(pl, t, -0.284496736f);
  pl = __builtin_fmaf(pl, t, 0.254829592f);
  pl *= t;
  const float e = __builtin_amdgcn_exp2f(-ax * ax * 1.4426950408889634f);
  const float er = __builtin_copysignf(1.0f - pl * e, v);
  return 0.5f * v * (1.0f + er);
}

// Plain-bf16 kernels only: GELU as x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3) -- |error| <= 4.8e-4 against the erf form, a
// sixteenth of the bf16 rounding the value (or the product it enters) receives next.  Two values at a time: the packed fp32
// multiply / fma / add take both in one instruction; 5 full-rate + 2 transcendental operations per value instead of 14 + 2.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 ff_gelu_sig2(f32x2 x) {
  const float A = -2.3022081f, B = -0.10294324f;       // -2 sqrt(2/pi) log2(e) * {1, 0.044715}
  const f32x2 x2 = x * x;
  const f32x2 pz = x2 * B + A;
  const f32x2 z = x * pz;
  f32x2 e;
  e[0] = __builtin_amdgcn_exp2f(z[0]); e[1] = __builtin_amdgcn_exp2f(z[1]);
  const f32x2 d = e + 1.0f;
  f32x2 r;
  r[0] = __builtin_amdgcn_rcpf(d[0]); r[1] = __builtin_amdgcn_rcpf(d[1]);
  return x * r;
}

__device__ __forceinline__ float ff_act_fast(float v, int act) { return act == ACT_GELU ? ff_gelu_fast(v) : ff_act(v, act); }

// compile-time activation (epilogues dispatch ONCE per kernel on the runtime code, not once per element:
// a per-element switch costs ~10 scalar+vector instructions and a branch for each of the 64-96 outputs of a lane)
template <int ACT, bool FAST>
__device__ __forceinline__ float ff_act_c(float v) {
  if (ACT == ACT_GELU) return FAST ? ff_gelu_fast(v) : 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
  if (ACT == ACT_RELU) return v > 0.f ? v : 0.f;
  if (ACT == ACT_LRELU) return v > 0.f ? v : 0.01f * v;
  if (ACT == ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
  return v;
}
template <int V> struct ff_ic { static constexpr int value = V; };
#define FF_DISPATCH_ACT(act, fn)                 \
  switch (act) {                                 \
    case ACT_GELU: fn(ff_ic<ACT_GELU>{}); break;       \
    case ACT_RELU: fn(ff_ic<ACT_RELU>{}); break;       \
    case ACT_LRELU: fn(ff_ic<ACT_LRELU>{}); break;     \
    case ACT_SIGMOID: fn(ff_ic<ACT_SIGMOID>{}); break; \
    default: fn(ff_ic<ACT_NONE>{}); break;             \
  }

// A wave reads its 32 token rows (K <= 192 floats each) COALESCED -- four 256-byte row segments per load instruction --
// and redistributes them through a wave-private LDS patch (32 rows x 68 dwords: 4-bank row shift, conflict-free
// ds_read_b128) into the MFMA B-operand order: v[st][j] = x[row l31][16 st + 8 hh + j].  Per-lane strided row reads
// (two lanes per row, 32 B per instruction and row) reach only ~1.7 TB/s; this form streams at the HBM rate.
template <int NPASS>   // (FF_XS_ROW: lds_layout.h)
__device__ __forceinline__ void ff_wave_rows_to_frags(const float* __restrict__ x, int ldx, long long tok0, long long M, int K,
                                                      float* xs, int lane, float (&v)[4 * NPASS][8]) {
  const int l31 = lane & 31, hh = lane >> 5;
  const int rr = lane >> 4, cq = (lane & 15) * 4;
  // every pass's loads are issued before the first one is consumed: one exposed HBM latency per wave instead of NPASS
  f32x4 t[NPASS][8];
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int r = 4 * j + rr, c = 64 * pass + cq;
      const bool ok = tok0 + r < M && c < K;
      const f32x4 u = *reinterpret_cast<const f32x4*>(x + (ok ? (tok0 + r) * ldx + c : 0));
      t[pass][j] = ok ? u : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
#pragma unroll
    for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(xs + (4 * j + rr) * FF_XS_ROW + cq) = t[pass][j];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(xs + l31 * FF_XS_ROW + 16 * s4 + 8 * hh);
      const f32x4 b = *reinterpret_cast<const f32x4*>(xs + l31 * FF_XS_ROW + 16 * s4 + 8 * hh + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[4 * pass + s4][e] = a[e]; v[4 * pass + s4][4 + e] = b[e]; }
    }
  }
}

// ---- LayerNorm on MFMA B fragments (the layout ff_wave_rows_to_frags leaves: v[st][j] = x[row l31][16 st + 8 hh + j]) ----------
// A LayerNorm or split change is made HERE -- and then carried to the sites that repeat this arithmetic inline, each for a
// measured reason stated at the site (registers, spills or time moved when the code went through the helpers):
//   token_linear_kernel.inc token_linear_kernel: statistics (the statistics helper costs an occupancy step)
//   frag_ln_opt_step.inc    token_linear_kernel, win_attn_fused_kernel: the step where gamma may be absent, the split and the xn side
//                           store -- ONE text for both
//   chan_qkv.hip            chan_qkv_kernel: statistics, step and split (slower through the helpers)
//   naf_tail.hip            naf_tail_kernel: statistics and step (slower through the helpers)
//   naf_fused.hip           naf_ffn_kernel: statistics, step and split (through the helpers the output bits moved)
//   naf_front.inc           naf_front_kernel: statistics, step and split (slower through the helpers)
//   naf_ln_stats.inc        the statistics of the three NAFNet kernels above with the compile-time channel count -- ONE text for them
//   win_attn_fused_v2_ln.inc      win_attn_fused_v2_kernel, hab_link_kernel: statistics and step (slower through the statistics helper)
//   token_projmlp_ln_stats.inc    token_projmlp_kernel, token_projmlp_bf16_kernel, hab_link_kernel: statistics in the ACCUMULATOR
//                                 layout (a helper spills; the bf16 step after it is token_projmlp_bf16_ln.inc)
// Callers: token_mlp_kernel (all three helpers), win_attn_fused_kernel (the corrected statistics; its step is frag_ln_opt_step.inc).
// Where K is a compile-time 16 KS (NAFNet) the k < K masks and the index clamps fold away.
// Statistics of a row over its K channels: plain sums in st-major order, the lane pair (l, l ^ 32) holds the row's two halves.
template <int KS>
__device__ __forceinline__ void ff_frag_ln_stats(const float (&v)[KS][8], int K, int hh, float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int st = 0; st < KS; ++st)
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[st][j];
  s += __shfl_xor(s, 32);
  mean = s / (float)K;
  float qv = 0.f;
#pragma unroll
  for (int st = 0; st < KS; ++st)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = (16 * st + 8 * hh + j < K) ? v[st][j] - mean : 0.f;
      qv += d * d;
    }
  qv += __shfl_xor(qv, 32);
  rstd = 1.0f / sqrtf(qv / (float)K + eps);
}

// The same, corrected two-pass (as win_attn_fused_v2_ln.inc): the residuals' own sum repairs the rounding of the first-pass mean.  On a
// (near-)constant row that rounding is all there is -- 0.1 in every channel came out 8.8e-6 from beta, (x - mean) * rstd with rstd = 316 --
// and there x - mean is exact, so the corrected mean is the row's value and the output is beta.  win_attn_fused_kernel only, whose
// normalised rows are held to 2e-6: token_mlp_kernel (held to 6e-5 on its output) goes from 234-238 VGPRs to 36 bytes of scratch with it.
template <int KS>
__device__ __forceinline__ void ff_frag_ln_stats_corrected(const float (&v)[KS][8], int K, int hh, float eps, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int st = 0; st < KS; ++st)
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[st][j];
  s += __shfl_xor(s, 32);
  mean = s / (float)K;
  float qv = 0.f, sd = 0.f;
#pragma unroll
  for (int st = 0; st < KS; ++st)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = (16 * st + 8 * hh + j < K) ? v[st][j] - mean : 0.f;
      qv += d * d;
      sd += d;
    }
  qv += __shfl_xor(qv, 32);
  sd += __shfl_xor(sd, 32);
  const float dm = sd / (float)K;
  mean += dm;
  rstd = 1.0f / sqrtf(fmaxf(qv / (float)K - dm * dm, 0.f) + eps);
}

// One k-step: f[j] = (v[j] - mean) * rstd * gamma[k0 + j] + beta[k0 + j], zero beyond K (k0 = 16 st + 8 hh).  The two float4
// loads per vector are clamped to index 0 beyond K: those values are unused.
__device__ __forceinline__ void ff_frag_ln_step(const float (&v)[8], const float* gamma, const float* beta, int k0, int K,
                                                float mean, float rstd, float (&f)[8]) {
  const int ka = k0 < K ? k0 : 0, kb = k0 + 4 < K ? k0 + 4 : 0;
  const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + ka), b0 = *reinterpret_cast<const f32x4*>(beta + ka);
  const f32x4 g1 = *reinterpret_cast<const f32x4*>(gamma + kb), b1 = *reinterpret_cast<const f32x4*>(beta + kb);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float gg = j < 4 ? g0[j & 3] : g1[j & 3], bb = j < 4 ? b0[j & 3] : b1[j & 3];
    f[j] = (k0 + j < K) ? (v[j] - mean) * rstd * gg + bb : 0.f;
  }
}

// split-bf16 operand pair: h + l carries 16 mantissa bits of f
__device__ __forceinline__ void ff_bf16_split(float f, __bf16& h, __bf16& l) {
  h = (__bf16)f;
  l = (__bf16)(f - (float)h);
}

// ---- the weight-tile MFMA loop of the token-stationary kernels ------------------------------------------------------------------
// A change to this loop is made HERE and carried to the three texts that repeat it for kernels whose assembly moved through the function:
//   token_linear_tile_mfma.inc          token_linear_kernel: gate GEMM and main tile loop
//   token_projmlp_bf16_tile_mfma.inc    token_projmlp_bf16_kernel, hab_link_kernel: projection and fc1 tile (hi plane only)
//   token_mlp_split_tile_mfma.inc       token_mlp_kernel, token_projmlp_kernel: the tokens' lo fragments read from LDS
// One 32-row weight tile in LDS times the wave's KS fragment steps, accumulated into acc.  ap is the lane's 16 bytes of k-step 0 in
// the tile's hi plane (row l31, + 16 hh; a k-step is 32 bytes further), the lo plane lies plane_bytes behind it.  NTERMS = 3 is the
// split-bf16 product hi.lo + lo.hi + hi.hi, NTERMS = 1 reads the hi plane only (xl and plane_bytes are then unused: pass xh, 0).
// swap = false: acc[weight row][token] (lane = token); true: acc[token][weight row].
// Operands are read TWO k-steps ahead (hipcc otherwise issues ds_read; s_waitcnt lgkmcnt(0); mfma per step and exposes the LDS
// latency at every step); the sched_barrier pair pins the read block in front of the MFMA block.
template <int KS, int NTERMS>
__device__ __forceinline__ void ff_tile_mfma(const unsigned char* ap, int plane_bytes, const bf16x8 (&xh)[KS], const bf16x8 (&xl)[KS],
                                             bool swap, f32x16& acc) {
  bf16x8 fa[2], fl[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    fa[u] = *reinterpret_cast<const bf16x8*>(ap + 32 * u);
    if (NTERMS == 3) fl[u] = *reinterpret_cast<const bf16x8*>(ap + 32 * u + plane_bytes);
  }
#pragma unroll
  for (int st = 0; st < KS; ++st) {
    const bf16x8 ah = fa[st & 1], al = fl[st & 1];
    if (st + 2 < KS) {
      fa[st & 1] = *reinterpret_cast<const bf16x8*>(ap + 32 * (st + 2));
      if (NTERMS == 3) fl[st & 1] = *reinterpret_cast<const bf16x8*>(ap + 32 * (st + 2) + plane_bytes);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (!swap) {
      if (NTERMS == 3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xl[st], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, xh[st], acc, 0, 0, 0);
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xh[st], acc, 0, 0, 0);
    } else {
      if (NTERMS == 3) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl[st], ah, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[st], al, acc, 0, 0, 0);
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[st], ah, acc, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// ---- small helpers shared by several files ---------------------------------------------------------------------------------
__device__ __forceinline__ float ff_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// exchanges bits 2 and 3 of a k index (the channel order in which prep.py stores the second GEMM's weights)
__device__ __forceinline__ int ff_swap23(int k) { return (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1); }

// lo <- the value held by lanes 0..31, hi <- the value held by lanes 32..63, in every lane (lane l and l ^ 32 pair up).
// v_permlane32_swap exchanges the upper half of its first operand with the lower half of its second; written as inline
// assembly because this toolchain's builtin returns the first result twice.  The s_nop pairs cover the VALU -> permlane and
// permlane -> VALU wait states the compiler's hazard recogniser would otherwise insert.
__device__ __forceinline__ void ff_halves(float v, float& lo, float& hi) {
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  lo = a; hi = b;
}

__device__ __forceinline__ int ff_reflect(int i, int n) {   // F.pad(mode='reflect') index map
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

__device__ __forceinline__ float ff_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

static inline int ff_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// Bijective XCD-aware block remap (guide section 5 T1): blocks with equal (bid % 8) share an XCD/L2,
// so give each XCD a contiguous run of logical tile ids.
__device__ __forceinline__ int ff_xcd_remap(int bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7;
  const int xcd = bid & 7, slot = bid >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + slot;
}
