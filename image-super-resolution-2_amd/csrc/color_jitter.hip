// The reference's paired colour jitter (augmentations.py:207-264, ColorJitter.__call__ / _apply_jitter) on a sampled micro-batch, in place:
// brightness, contrast around the patch mean, and -- unless the factor is exactly 1 -- saturation through the 8-bit HSV conversion that
// cv2.cvtColor(COLOR_RGB2HSV / COLOR_HSV2RGB) is published to be (12-bit fixed-point forward, fp32 sector table backward).  The LR and the
// HR patch of a sample share the three factors; each uses its OWN mean.
//
//   lr [B][3][p][p], hr [B][3][4p][4p]   fp32 = u / 255 (IEEE division, u a byte): what ff_sample_pairs_u8 writes
//   table DEVICE fp32 [B][4] = {apply, bf, cf, sf}; apply == 0 leaves both patches of the sample untouched
//
// Two launches.
//   cj_sum_kernel     S = the exact integer sum of a patch's 3 P P bytes u = rint(255 x): CJ_PARTS workgroups per (sample, tensor), each
//                     writing one 64-bit partial (no atomics, nothing to zero; integer, so the order does not matter).
//   cj_apply_kernel   one workgroup = CJ_CHUNK consecutive pixels of one patch, a pixel's three planes together:
//                       mean = float( double(bf) * ( double(S) / (255.0 * 3 P P) ) )        -- (img * bf).mean() by exact summation
//                       x2   = (x * bf - mean) * cf + mean
//                       sf == 1:  out = min(max(x2, 0), 1)                                  -- no quantisation (`if saturation != 1.0`)
//                       else:     q = (u8) trunc(clip(x2) * 255); (H, S, V) = rgb2hsv8(q); S' = (u8) trunc(clip(float(S) * sf, 0, 255));
//                                 out = hsv2rgb8(H, S', V) / 255
//                     rgb2hsv8: v = max, d = v - min, S = (d sdiv[v] + 2048) >> 12, H = (h hdiv[d] + 2048) >> 12 (+180 when negative) with
//                     h = g - b | b - r + 2d | r - g + 4d by the channel that holds v, sdiv[i] = rint(255 * 4096 / i), hdiv[i] = rint(180 *
//                     4096 / (6 i)), ties to even.  The two tables are made per workgroup in LDS by exact integer arithmetic.
//                     hsv2rgb8: hh = H * (6/180), s = S' / 255, vv = V / 255 as fp32 products with the rounded reciprocals; sector = floor(hh),
//                     f = hh - sector; tab = {vv, vv (1 - s), vv (1 - s f), vv (1 - s (1 - f))} picked per sector; byte = rint(255 c).
// Every fp32 step is a separately rounded operation (contraction is OFF in this file: a fused multiply-add would change the bits), the
// mean is fp64.  A workgroup's sample -- hence its apply flag and its sf -- is uniform, so no barrier is skipped by part of a group.
// p % 4 == 0 and 16-byte aligned tensors: float4 loads and stores; otherwise one float at a time.  Offsets and sums are 64-bit.
#include "ff_common.h"

#pragma clang fp contract(off)

#define CJ_PARTS 16
#define CJ_CHUNK 1024

__device__ __forceinline__ unsigned cj_byte(float x) { return (unsigned)__builtin_rintf(x * 255.0f); }

// rint(n / d) for positive integers, ties to even
__device__ __forceinline__ int cj_rdiv(int n, int d) {
  const int q = n / d, r2 = 2 * (n - q * d);
  return q + ((r2 > d || (r2 == d && (q & 1))) ? 1 : 0);
}

template <bool VEC>
__global__ __launch_bounds__(256) void cj_sum_kernel(const float* __restrict__ lr, const float* __restrict__ hr, const float* __restrict__ table,
                                                     int p, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long ws[4];
  const int b = blockIdx.x / (2 * CJ_PARTS), r_ = blockIdx.x - b * (2 * CJ_PARTS);
  const int is_hr = r_ / CJ_PARTS, k = r_ - is_hr * CJ_PARTS;
  if (table[4ll * b] == 0.f) return;                           // uniform per workgroup
  const long long P = is_hr ? 4ll * p : (long long)p, n = 3 * P * P;
  const float* src = (is_hr ? hr : lr) + (long long)b * n;
  const int tid = threadIdx.x;
  unsigned long long s = 0;
  if (VEC) {                                                   // n % 4 == 0
    for (long long i = k * 256 + tid; i < n / 4; i += CJ_PARTS * 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * i);
      s += (cj_byte(v[0]) + cj_byte(v[1])) + (cj_byte(v[2]) + cj_byte(v[3]));
    }
  } else {
    for (long long i = k * 256 + tid; i < n; i += CJ_PARTS * 256) s += cj_byte(src[i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) ws[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// one pixel, in place in (r, g, b)
__device__ __forceinline__ void cj_pixel(float& r, float& g, float& b, float bf, float cf, float sf, float mean, bool sat, const int* tab) {
  float x[3] = {r, g, b};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x1 = x[c] * bf;
    const float x2 = (x1 - mean) * cf + mean;
    x[c] = fminf(fmaxf(x2, 0.f), 1.f);
  }
  if (!sat) {
    r = x[0]; g = x[1]; b = x[2];
    return;
  }
  const int qr = (int)(x[0] * 255.0f), qg = (int)(x[1] * 255.0f), qb = (int)(x[2] * 255.0f);      // trunc; 0..255
  const int v = max(qr, max(qg, qb)), m = min(qr, min(qg, qb)), d = v - m;
  const int S = (d * tab[v] + 2048) >> 12;
  const int h = v == qr ? qg - qb : (v == qg ? qb - qr + 2 * d : qr - qg + 4 * d);
  int H = (h * tab[256 + d] + 2048) >> 12;                     // arithmetic shift: h may be negative
  if (H < 0) H += 180;
  const int S2 = (int)fminf(fmaxf((float)S * sf, 0.f), 255.f);
  const float vv = (float)v * (1.f / 255.f);
  float cr = vv, cg = vv, cb = vv;
  if (S2 != 0) {
    const float hh = (float)H * (6.f / 180.f), s = (float)S2 * (1.f / 255.f);
    const float fl = floorf(hh);
    const float f = hh - fl;
    const int sec = ((int)fl) % 6;
    const float t1 = vv * (1.f - s), t2 = vv * (1.f - s * f), t3 = vv * (1.f - s * (1.f - f));
    // (b, g, r) = tab[idx[sec]], idx = {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}}, tab = {vv, t1, t2, t3}
    cb = sec == 0 || sec == 1 ? t1 : (sec == 2 ? t3 : (sec == 5 ? t2 : vv));
    cg = sec == 0 ? t3 : (sec == 1 || sec == 2 ? vv : (sec == 3 ? t2 : t1));
    cr = sec == 0 || sec == 5 ? vv : (sec == 1 ? t2 : (sec == 4 ? t3 : t1));
  }
  r = __fdiv_rn(fminf(fmaxf(__builtin_rintf(cr * 255.f), 0.f), 255.f), 255.0f);
  g = __fdiv_rn(fminf(fmaxf(__builtin_rintf(cg * 255.f), 0.f), 255.f), 255.0f);
  b = __fdiv_rn(fminf(fmaxf(__builtin_rintf(cb * 255.f), 0.f), 255.f), 255.0f);
}

template <bool VEC>
__global__ __launch_bounds__(256) void cj_apply_kernel(float* __restrict__ lr, float* __restrict__ hr, const float* __restrict__ table, int p,
                                                       const unsigned long long* __restrict__ part, int chunks_lr, int chunks_hr) {
  __shared__ int tab[512];                                     // sdiv[256], hdiv[256]
  const int per = chunks_lr + chunks_hr;
  const int b = blockIdx.x / per, r_ = blockIdx.x - b * per;
  const float* row = table + 4ll * b;
  if (row[0] == 0.f) return;                                   // uniform per workgroup: the barrier below is reached by all or by none
  const float bf = row[1], cf = row[2], sf = row[3];
  const int is_hr = r_ >= chunks_lr;
  const long long ch = is_hr ? r_ - chunks_lr : r_;
  const long long P = is_hr ? 4ll * p : (long long)p, plane = P * P;
  float* base = (is_hr ? hr : lr) + (long long)b * 3 * plane;
  const unsigned long long* pp = part + ((long long)b * 2 + is_hr) * CJ_PARTS;
  unsigned long long S = 0;
#pragma unroll
  for (int k = 0; k < CJ_PARTS; ++k) S += pp[k];
  const float mean = (float)((double)bf * ((double)S / (255.0 * (double)(3 * plane))));
  const int tid = threadIdx.x;
  const bool sat = sf != 1.0f;
  if (sat) {                                                   // uniform
    tab[tid] = tid ? cj_rdiv(255 * 4096, tid) : 0;
    tab[256 + tid] = tid ? cj_rdiv(180 * 4096, 6 * tid) : 0;
    __syncthreads();
  }
  if (VEC) {                                                   // plane % 4 == 0: a group of four never straddles the end
    const long long i = 4 * (ch * (CJ_CHUNK / 4) + tid);
    if (i < plane) {
      f32x4 v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const f32x4*>(base + c * plane + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float r = v[0][j], g = v[1][j], bl = v[2][j];
        cj_pixel(r, g, bl, bf, cf, sf, mean, sat, tab);
        v[0][j] = r; v[1][j] = g; v[2][j] = bl;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(base + c * plane + i) = v[c];
    }
  } else {
#pragma unroll
    for (int j = 0; j < CJ_CHUNK / 256; ++j) {
      const long long i = ch * CJ_CHUNK + j * 256 + tid;
      if (i < plane) {
        float r = base[i], g = base[plane + i], bl = base[2 * plane + i];
        cj_pixel(r, g, bl, bf, cf, sf, mean, sat, tab);
        base[i] = r; base[plane + i] = g; base[2 * plane + i] = bl;
      }
    }
  }
}

extern "C" long long ff_color_jitter_workspace(int B) { return B < 1 ? -1 : (long long)B * 2 * CJ_PARTS * (long long)sizeof(unsigned long long); }

extern "C" int ff_color_jitter_pairs(float* lr, float* hr, const float* table, int B, int p, void* workspace, long long workspace_bytes,
                                     void* stream) {
  FF_CHECK_ARG(lr && hr && table && workspace && B >= 1 && p >= 1,
               "ff_color_jitter_pairs: null pointer or bad sizes (B %d, p %d: both must be >= 1)", B, p);
  FF_CHECK_ARG(p <= 8192 && B <= (1 << 20), "ff_color_jitter_pairs: sizes out of range (B %d, p %d)", B, p);
  FF_CHECK_ARG(workspace_bytes >= ff_color_jitter_workspace(B) && (((uintptr_t)workspace) & 7) == 0,
               "ff_color_jitter_pairs: workspace of %lld bytes, need %lld (8-byte aligned)", workspace_bytes, ff_color_jitter_workspace(B));
  const int ch_lr = ff_cdiv((long long)p * p, CJ_CHUNK), ch_hr = ff_cdiv(16ll * p * p, CJ_CHUNK);
  const long long blocks = (long long)B * ((long long)ch_lr + ch_hr);
  FF_CHECK_ARG(blocks < (1ll << 31), "ff_color_jitter_pairs: %lld chunks exceed the grid limit", blocks);
  unsigned long long* part = (unsigned long long*)workspace;
  // float4 access needs planes of whole groups in BOTH tensors (p % 4 == 0) and 16-byte aligned tensors; else the dword form
  const bool vec = p % 4 == 0 && ((((uintptr_t)lr) | ((uintptr_t)hr)) & 15) == 0;
  const dim3 g1((unsigned)(B * 2 * CJ_PARTS)), g2((unsigned)blocks);
  if (vec) {
    hipLaunchKernelGGL(cj_sum_kernel<true>, g1, dim3(256), 0, (hipStream_t)stream, lr, hr, table, p, part);
    hipLaunchKernelGGL(cj_apply_kernel<true>, g2, dim3(256), 0, (hipStream_t)stream, lr, hr, table, p, part, ch_lr, ch_hr);
  } else {
    hipLaunchKernelGGL(cj_sum_kernel<false>, g1, dim3(256), 0, (hipStream_t)stream, lr, hr, table, p, part);
    hipLaunchKernelGGL(cj_apply_kernel<false>, g2, dim3(256), 0, (hipStream_t)stream, lr, hr, table, p, part, ch_lr, ch_hr);
  }
  FF_LAUNCH_CHECK("ff_color_jitter_pairs");
  return FF_OK;
}
