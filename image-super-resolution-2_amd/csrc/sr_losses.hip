// The reference's staged training losses (src/losses/perceptual_loss.py, CombinedLoss.forward :1207-1283) on HIP.
// Every component takes the pre-clamp prediction `sr` and the target `hr`, both NHWC [B][H][W][3] fp32 (train.py:325 clamps
// before the criterion), and produces
//   value[0]  = the UNWEIGHTED component value (a device scalar; CombinedLoss's `return_components` entry), and
//   dsr      (+)= weight * d(value)/d(sr) with the inclusive clamp mask 0 <= sr <= 1 of l1_stage1_kernel (dsr may be null).
// Reductions: per-workgroup partials in a fixed assignment, added by loss_finish_kernel in a fixed order; no float atomics, so
// two identical calls give identical bits.
//   ff_loss_pointwise  l1 / charbonnier (eps 1e-6) / l2                 perceptual_loss.py:68-195
//   ff_loss_ssim       1 - mean SSIM map, 11x11 Gaussian (sigma 1.5), zero padding 5, per channel   :197-295
//   ff_loss_edge       l1(Sobel x) + l1(Sobel y), zero padding 1         :996-1049
//   ff_loss_swt        haar, 2 levels, the GPU approximation (reflect pad 2^l, dilated 2x2 filters)  :617-813, :1138-1142
//   ff_loss_fft        mean(w |‖P‖-‖T‖|) + 0.1 mean(w |∠P-∠T|), P = fft2(pred, 'ortho'), w = 1 + dist/maxdist  :506-600
//   ff_loss_combine    total = sum_k weight_k * value_k in CombinedLoss's order (sequential fp32, as the reference adds)
#include "ff_common.h"

extern "C" int ff_rfft2(const float* x, int C, int H, int W, const float* twW_cos, const float* twW_sin, const float* twH_cos,
                        const float* twH_sin, float* work, long long work_floats, float* spec, void* stream);
extern "C" int ff_irfft2(const float* spec, int C, int H, int W, const float* twW_cos, const float* twW_sin, const float* twH_cos,
                         const float* twH_sin, float* work, long long work_floats, float* out, void* stream);

#define LS_NB 1024                                  // grid of the grid-stride kernels = number of partials

__device__ __forceinline__ float ls_mask(float x) { return (x >= 0.f && x <= 1.f) ? 1.f : 0.f; }
__device__ __forceinline__ float ls_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ void ls_put(float* __restrict__ dsr, long long i, float g, int acc) { dsr[i] = acc ? dsr[i] + g : g; }

// 256-thread tree sum in a fixed order; every thread gets the result
__device__ __forceinline__ float ls_block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// out[0] = bias + scale * sum(part[0..n))
__global__ __launch_bounds__(256) void loss_finish_kernel(const float* __restrict__ part, int n, float scale, float bias,
                                                          float* __restrict__ out) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  s = ls_block_sum(s, red);
  if (threadIdx.x == 0) out[0] = bias + s * scale;
}

static int ls_blocks(long long n) { return (int)((n + 255) / 256 < LS_NB ? (n + 255) / 256 : LS_NB); }

// ------------------------------------------------------------------------------------------------------------------ pointwise
// kind 0: |d|, grad sign(d);  kind 1: sqrt(d^2 + eps^2), grad d / sqrt(..);  kind 2: d^2, grad 2d   (d = clamp(sr) - hr)
__global__ __launch_bounds__(256) void pointwise_loss_kernel(int kind, const float* __restrict__ sr, const float* __restrict__ hr,
                                                             float* __restrict__ dsr, int acc, long long n, float gscale,
                                                             float* __restrict__ part) {
  __shared__ float red[256];
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float x = sr[i], d = ff_clamp01(x) - hr[i];
    float v, g;
    if (kind == 0) { v = fabsf(d); g = ls_sign(d); }
    else if (kind == 1) { v = sqrtf(d * d + 1e-12f); g = d / v; }
    else { v = d * d; g = 2.f * d; }
    s += v;
    if (dsr) ls_put(dsr, i, gscale * ls_mask(x) * g, acc);
  }
  s = ls_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------------------------ SSIM
// The tiling of ssim_map_kernel (csrc/metrics.hip): one workgroup = a 16x16 tile of one channel plane, 26x26 patches in LDS,
// separable 11-tap Gaussian.  Pass 1 forms the five filtered maps and, per pixel, S and the three coefficient maps
//   ca = dS/dmu1, cb = dS/dE[x^2], cc = dS/dE[xy]            (mu1, E[.] are the filtered maps; sigma = E - mu mu)
// Pass 2 filters the coefficient maps with the same (symmetric, zero-padded) window:
//   dL/dx = -(1/n) (G*ca + 2 x G*cb + y G*cc)
#define LS_T 16
#define LS_R 5
#define LS_P (LS_T + 2 * LS_R)
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ sr, const float* __restrict__ hr, int H, int W,
                                                       const float* __restrict__ gw, float* __restrict__ coef, float* __restrict__ part) {
  __shared__ float pa[LS_P][LS_P + 1], pb[LS_P][LS_P + 1];
  __shared__ float hq[5][LS_P][LS_T + 1];
  __shared__ float g[11];
  __shared__ float red[256];
  const int tx = blockIdx.x, ty = blockIdx.y, b = blockIdx.z / 3, c = blockIdx.z % 3;
  const int tid = threadIdx.x;
  if (tid < 11) g[tid] = gw[tid];
  for (int i = tid; i < LS_P * LS_P; i += 256) {
    const int ly = i / LS_P, lx = i % LS_P;
    const int y = ty * LS_T + ly - LS_R, x = tx * LS_T + lx - LS_R;
    float va = 0.f, vb = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const long long o = (((long long)b * H + y) * W + x) * 3 + c;
      va = ff_clamp01(sr[o]);
      vb = hr[o];
    }
    pa[ly][lx] = va;
    pb[ly][lx] = vb;
  }
  __syncthreads();
  for (int i = tid; i < LS_P * LS_T; i += 256) {
    const int ly = i / LS_T, lx = i % LS_T;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float va = pa[ly][lx + k], vb = pb[ly][lx + k], wk = g[k];
      s0 += wk * va; s1 += wk * vb; s2 += wk * (va * va); s3 += wk * (vb * vb); s4 += wk * (va * vb);
    }
    hq[0][ly][lx] = s0; hq[1][ly][lx] = s1; hq[2][ly][lx] = s2; hq[3][ly][lx] = s3; hq[4][ly][lx] = s4;
  }
  __syncthreads();
  const int ly = tid / LS_T, lx = tid % LS_T;
  const int oy = ty * LS_T + ly, ox = tx * LS_T + lx;
  float v = 0.f;
  if (oy < H && ox < W) {
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float wk = g[k];
      m1 += wk * hq[0][ly + k][lx]; m2 += wk * hq[1][ly + k][lx];
      e11 += wk * hq[2][ly + k][lx]; e22 += wk * hq[3][ly + k][lx]; e12 += wk * hq[4][ly + k][lx];
    }
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
    const float s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
    const float A1 = 2.f * m12 + C1, A2 = 2.f * s12 + C2, B1 = m11 + m22 + C1, B2 = s11 + s22 + C2;
    const float den = B1 * B2, S = (A1 * A2) / den;
    v = S;
    if (coef) {
      const long long P = (long long)H * W, o = (long long)blockIdx.z * P + (long long)oy * W + ox;
      coef[o] = 2.f * m2 * (A2 - A1) / den - 2.f * m1 * S * (1.f / B1 - 1.f / B2);
      coef[(long long)gridDim.z * P + o] = -S / B2;
      coef[2LL * gridDim.z * P + o] = 2.f * A1 / den;
    }
  }
  v = ls_block_sum(v, red);
  if (tid == 0) part[((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = v;
}

__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ sr, const float* __restrict__ hr, int H, int W,
                                                       const float* __restrict__ gw, const float* __restrict__ coef, float gscale,
                                                       float* __restrict__ dsr, int acc) {
  __shared__ float pc[3][LS_P][LS_P + 1];
  __shared__ float hq[3][LS_P][LS_T + 1];
  __shared__ float g[11];
  const int tx = blockIdx.x, ty = blockIdx.y, b = blockIdx.z / 3, c = blockIdx.z % 3;
  const int tid = threadIdx.x;
  const long long P = (long long)H * W, plane = (long long)gridDim.z * P;
  if (tid < 11) g[tid] = gw[tid];
  for (int i = tid; i < LS_P * LS_P; i += 256) {
    const int ly = i / LS_P, lx = i % LS_P;
    const int y = ty * LS_T + ly - LS_R, x = tx * LS_T + lx - LS_R;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const long long o = (long long)blockIdx.z * P + (long long)y * W + x;
      v0 = coef[o]; v1 = coef[plane + o]; v2 = coef[2 * plane + o];
    }
    pc[0][ly][lx] = v0; pc[1][ly][lx] = v1; pc[2][ly][lx] = v2;
  }
  __syncthreads();
  for (int i = tid; i < LS_P * LS_T; i += 256) {
    const int ly = i / LS_T, lx = i % LS_T;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float wk = g[k];
      s0 += wk * pc[0][ly][lx + k]; s1 += wk * pc[1][ly][lx + k]; s2 += wk * pc[2][ly][lx + k];
    }
    hq[0][ly][lx] = s0; hq[1][ly][lx] = s1; hq[2][ly][lx] = s2;
  }
  __syncthreads();
  const int ly = tid / LS_T, lx = tid % LS_T;
  const int oy = ty * LS_T + ly, ox = tx * LS_T + lx;
  if (oy < H && ox < W) {
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float wk = g[k];
      f0 += wk * hq[0][ly + k][lx]; f1 += wk * hq[1][ly + k][lx]; f2 += wk * hq[2][ly + k][lx];
    }
    const long long o = (((long long)b * H + oy) * W + ox) * 3 + c;
    const float xs = sr[o], xv = ff_clamp01(xs), yv = hr[o];
    ls_put(dsr, o, -gscale * ls_mask(xs) * (f0 + 2.f * xv * f1 + yv * f2), acc);
  }
}

// ------------------------------------------------------------------------------------------------------------------ edge
// gx = Kx * D, gy = Ky * D with D = clamp(sr) - hr (the Sobel operator is linear), zero padding 1, per channel.
// Pass 1: sum |gx| + |gy| and the signs; pass 2: the adjoint (correlation with the flipped taps) of the signs.
__device__ __forceinline__ float ls_kx(int i, int j) { return (float)((j - 1) * (i == 1 ? 2 : 1)); }   // [[-1,0,1],[-2,0,2],[-1,0,1]]
__device__ __forceinline__ float ls_ky(int i, int j) { return (float)((i - 1) * (j == 1 ? 2 : 1)); }   // [[-1,-2,-1],[0,0,0],[1,2,1]]

__global__ __launch_bounds__(256) void edge_fwd_kernel(const float* __restrict__ sr, const float* __restrict__ hr, int B, int H, int W,
                                                       float* __restrict__ sgn, float* __restrict__ part) {
  __shared__ float red[256];
  const long long n = (long long)B * H * W * 3;
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const long long p = i / 3;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long long b = p / ((long long)W * H);
    float gx = 0.f, gy = 0.f;
#pragma unroll
    for (int ki = 0; ki < 3; ++ki) {
      const int yy = y + ki - 1;
      if (yy < 0 || yy >= H) continue;
#pragma unroll
      for (int kj = 0; kj < 3; ++kj) {
        const int xx = x + kj - 1;
        if (xx < 0 || xx >= W) continue;
        const long long o = ((b * H + yy) * W + xx) * 3 + c;
        const float d = ff_clamp01(sr[o]) - hr[o];
        gx += ls_kx(ki, kj) * d;
        gy += ls_ky(ki, kj) * d;
      }
    }
    s += fabsf(gx) + fabsf(gy);
    if (sgn) { sgn[i] = ls_sign(gx); sgn[n + i] = ls_sign(gy); }
  }
  s = ls_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void edge_bwd_kernel(const float* __restrict__ sr, int B, int H, int W, const float* __restrict__ sgn,
                                                       float gscale, float* __restrict__ dsr, int acc) {
  const long long n = (long long)B * H * W * 3;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const long long p = i / 3;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long long b = p / ((long long)W * H);
    float g = 0.f;
#pragma unroll
    for (int ki = 0; ki < 3; ++ki) {
      const int yy = y - ki + 1;                        // the output pixel whose tap (ki, kj) reads (y, x)
      if (yy < 0 || yy >= H) continue;
#pragma unroll
      for (int kj = 0; kj < 3; ++kj) {
        const int xx = x - kj + 1;
        if (xx < 0 || xx >= W) continue;
        const long long o = ((b * H + yy) * W + xx) * 3 + c;
        g += ls_kx(ki, kj) * sgn[o] + ls_ky(ki, kj) * sgn[n + o];
      }
    }
    ls_put(dsr, i, gscale * ls_mask(sr[i]) * g, acc);
  }
}

// ------------------------------------------------------------------------------------------------------------------ SWT
// SWTLoss._swt2d_gpu with haar (dec_lo = [h, h], dec_hi = [-h, h], h = 1/sqrt 2), level 2: at level l (dilation d = 2^l) the
// reflect-padded (pad d), cropped [:H, :W] correlation with a 2x2 filter f reads cur[R(y - d + i d)][R(x - d + j d)], i, j in {0,1},
// R(k) = |k| (the crop keeps only the top / left reflection).  Bands in the filters' stacking order (:661-682):
//   a: lo[i] lo[j]   h: hi[i] lo[j]   v: lo[i] hi[j]   d: hi[i] hi[j]       (i: row tap, j: column tap)
// loss = (1/levels) sum_l sum_band w_band mean |P_band - T_band|, w = (a 0.5, h 1.5, v 1.5, d 2.0); cA of level 0 feeds level 1.
// Pass 1: level 0 (partials, cA0 of both images, weighted signs s0); pass 2: level 1 (partials, weighted signs s1); pass 3: the
// level-1 adjoint of s1 added into s0[a]; pass 4: the level-0 adjoint of s0 -> dsr.
__constant__ float kSwtW[4] = {0.5f, 1.5f, 1.5f, 2.0f};

__device__ __forceinline__ float ls_haar(int hi, int t) {
  const float h = 0.7071067811865476f;
  return hi ? (t ? h : -h) : h;
}
// filter tap of band k at (i, j), formed as the reference forms it: a product of two fp32 values
__device__ __forceinline__ float ls_swt_f(int k, int i, int j) {
  const int hr_ = (k == 1 || k == 3), hc = (k == 2 || k == 3);
  return ls_haar(hc, j) * ls_haar(hr_, i);
}

// one level at pixel p = (b, y, x, c) of a NHWC image `cur` (values via ld): four bands
template <typename LD>
__device__ __forceinline__ void ls_swt_bands(LD ld, long long b, int y, int x, int c, int H, int W, int d, float out[4]) {
  float v[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int yy = abs(y - d + i * d), xx = abs(x - d + j * d);
      v[i][j] = ld(((b * H + yy) * W + xx) * 3 + c);
    }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) s += ls_swt_f(k, i, j) * v[i][j];
    out[k] = s;
  }
}

// the (output position, tap) pairs whose read lands on source position r along one axis of length N at dilation d
__device__ __forceinline__ int ls_swt_adj(int r, int d, int N, int* pos, int* tap) {
  int m = 0;
  pos[m] = r; tap[m++] = 1;                             // y = r, tap 1 reads y
  if (r + d < N) { pos[m] = r + d; tap[m++] = 0; }      // y - d = r
  if (r > 0 && r <= d && d - r < N) { pos[m] = d - r; tap[m++] = 0; }   // y - d = -r (reflected)
  return m;
}

__global__ __launch_bounds__(256) void swt_l0_kernel(const float* __restrict__ sr, const float* __restrict__ hr, int B, int H, int W,
                                                     float* __restrict__ cA, float* __restrict__ s0, float* __restrict__ part) {
  __shared__ float red[256];
  const long long n = (long long)B * H * W * 3;
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const long long p = i / 3;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long long b = p / ((long long)W * H);
    float bp[4], bt[4];
    ls_swt_bands([&](long long o) { return ff_clamp01(sr[o]); }, b, y, x, c, H, W, 1, bp);
    ls_swt_bands([&](long long o) { return hr[o]; }, b, y, x, c, H, W, 1, bt);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dd = bp[k] - bt[k];
      s += kSwtW[k] * fabsf(dd);
      if (s0) s0[k * n + i] = kSwtW[k] * ls_sign(dd);
    }
    cA[i] = bp[0];
    cA[n + i] = bt[0];
  }
  s = ls_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void swt_l1_kernel(const float* __restrict__ cA, int B, int H, int W, float* __restrict__ s1,
                                                     float* __restrict__ part) {
  __shared__ float red[256];
  const long long n = (long long)B * H * W * 3;
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const long long p = i / 3;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long long b = p / ((long long)W * H);
    float bp[4], bt[4];
    ls_swt_bands([&](long long o) { return cA[o]; }, b, y, x, c, H, W, 2, bp);
    ls_swt_bands([&](long long o) { return cA[n + o]; }, b, y, x, c, H, W, 2, bt);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dd = bp[k] - bt[k];
      s += kSwtW[k] * fabsf(dd);
      if (s1) s1[k * n + i] = kSwtW[k] * ls_sign(dd);
    }
  }
  s = ls_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// adjoint of one level (dilation d) of the band signals s[4][n] at source pixel i
__device__ __forceinline__ float ls_swt_adjoint(const float* __restrict__ s, long long n, long long i, int H, int W, int d) {
  const int c = (int)(i % 3);
  const long long p = i / 3;
  const int x = (int)(p % W), y = (int)((p / W) % H);
  const long long b = p / ((long long)W * H);
  int py[3], ti[3], px[3], tj[3];
  const int my = ls_swt_adj(y, d, H, py, ti), mx = ls_swt_adj(x, d, W, px, tj);
  float g = 0.f;
  for (int u = 0; u < my; ++u)
    for (int v = 0; v < mx; ++v) {
      const long long o = ((b * H + py[u]) * W + px[v]) * 3 + c;
#pragma unroll
      for (int k = 0; k < 4; ++k) g += ls_swt_f(k, ti[u], tj[v]) * s[k * n + o];
    }
  return g;
}

__global__ __launch_bounds__(256) void swt_adj1_kernel(const float* __restrict__ s1, int B, int H, int W, float* __restrict__ s0a) {
  const long long n = (long long)B * H * W * 3;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    s0a[i] += ls_swt_adjoint(s1, n, i, H, W, 2);
}

__global__ __launch_bounds__(256) void swt_adj0_kernel(const float* __restrict__ sr, const float* __restrict__ s0, int B, int H, int W,
                                                       float gscale, float* __restrict__ dsr, int acc) {
  const long long n = (long long)B * H * W * 3;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    ls_put(dsr, i, gscale * ls_mask(sr[i]) * ls_swt_adjoint(s0, n, i, H, W, 1), acc);
}

// ------------------------------------------------------------------------------------------------------------------ FFT
// P = fft2(clamp(sr), 'ortho') per plane from the half spectrum of ff_rfft2 (csrc/freq.hip).  The full-spectrum sum is the half
// sum with multiplicity 2 for the columns that have a conjugate partner (the weight is symmetric under (u,v) -> (-u,-v), and so are
// both terms).  The four self-conjugate bins get an imaginary part of exactly +0, as torch's r2c gives them (a rounding residue
// would turn atan2's +pi into -pi there).  The gradient spectrum, WITHOUT the multiplicity, is written over P: the adjoint of the
// ortho transform of a real image is Re(F^H g) = irfft2(g_half) for a Hermitian g -- c2r doubles the paired columns itself.
__global__ __launch_bounds__(256) void nhwc_to_planes_kernel(const float* __restrict__ sr, const float* __restrict__ hr, long long n, int HW,
                                                             float* __restrict__ P, float* __restrict__ T) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const long long p = i / 3, b = p / HW, o = (b * 3 + c) * HW + p % HW;
    P[o] = ff_clamp01(sr[i]);
    T[o] = hr[i];
  }
}

__global__ __launch_bounds__(256) void fft_loss_kernel(float* __restrict__ SP, const float* __restrict__ ST, int planes, int H, int W,
                                                       float maxd, float gscale, int want_grad, float* __restrict__ part) {
  __shared__ float red[256];
  const int Wf = W / 2 + 1;
  const long long nb = (long long)planes * H * Wf;
  float s = 0.f;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nb; e += (long long)gridDim.x * 256) {
    const int v = (int)(e % Wf), u = (int)((e / Wf) % H);
    float pr = SP[2 * e], pi = SP[2 * e + 1], tr = ST[2 * e], ti = ST[2 * e + 1];
    const bool vself = v == 0 || 2 * v == W;
    if (vself && (u == 0 || 2 * u == H)) { pi = 0.f; ti = 0.f; }
    const float dy = (float)((u + H / 2) % H - H / 2), dx = (float)((v + W / 2) % W - W / 2);   // after fftshift
    const float wq = 1.0f + 1.0f * (sqrtf(dx * dx + dy * dy) / maxd);
    const float mp = sqrtf(pr * pr + pi * pi), mt = sqrtf(tr * tr + ti * ti);
    const float ap = atan2f(pi, pr), at = atan2f(ti, tr);
    s += (vself ? 1.f : 2.f) * (wq * fabsf(mp - mt) + 0.1f * (wq * fabsf(ap - at)));
    if (want_grad) {
      float gr = 0.f, gi = 0.f;
      if (mp > 0.f) {
        const float sm = ls_sign(mp - mt) / mp, sa = 0.1f * ls_sign(ap - at) / (mp * mp);
        gr = gscale * wq * (sm * pr - sa * pi);
        gi = gscale * wq * (sm * pi + sa * pr);
      }
      SP[2 * e] = gr;
      SP[2 * e + 1] = gi;
    }
  }
  s = ls_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void planes_to_nhwc_grad_kernel(const float* __restrict__ sr, const float* __restrict__ G, long long n,
                                                                  int HW, float* __restrict__ dsr, int acc) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const long long p = i / 3, b = p / HW, o = (b * 3 + c) * HW + p % HW;
    ls_put(dsr, i, ls_mask(sr[i]) * G[o], acc);
  }
}

// ------------------------------------------------------------------------------------------------------------------ entry points
enum { LS_L1 = 0, LS_CHARB = 1, LS_L2 = 2, LS_SSIM = 3, LS_EDGE = 4, LS_SWT = 5, LS_FFT = 6 };

extern "C" long long ff_loss_workspace(int component, int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return -1;
  const long long n = (long long)B * H * W * 3;
  switch (component) {
    case LS_L1: case LS_CHARB: case LS_L2: return LS_NB;
    case LS_SSIM: return 3 * n + (long long)B * 3 * ff_cdiv(H, LS_T) * ff_cdiv(W, LS_T);
    case LS_EDGE: return 2 * n + LS_NB;
    case LS_SWT: return 10 * n + 2 * LS_NB;
    case LS_FFT: return 2 * n + 3 * (long long)B * 3 * H * (W / 2 + 1) * 2 + LS_NB;
    default: return -1;
  }
}

#define LS_ARGS_OK(name)                                                                                                  \
  FF_CHECK_ARG(sr && hr && value && work && B > 0 && H > 0 && W > 0, name ": bad args");                                  \
  FF_CHECK_ARG(work_floats >= ff_loss_workspace(comp, B, H, W), name ": workspace too small (need %lld floats)",         \
               ff_loss_workspace(comp, B, H, W))

extern "C" int ff_loss_pointwise(int kind, const float* sr, const float* hr, int B, int H, int W, float weight, float* dsr, int accumulate,
                                 float* value, float* work, long long work_floats, void* stream) {
  const int comp = kind;
  FF_CHECK_ARG(kind >= 0 && kind <= 2, "ff_loss_pointwise: kind must be 0 (l1), 1 (charbonnier) or 2 (l2)");
  LS_ARGS_OK("ff_loss_pointwise");
  const long long n = (long long)B * H * W * 3;
  const int nb = ls_blocks(n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pointwise_loss_kernel, dim3(nb), dim3(256), 0, st, kind, sr, hr, dsr, accumulate, n, weight / (float)n, work);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, work, nb, 1.0f / (float)n, 0.f, value);
  FF_LAUNCH_CHECK("ff_loss_pointwise");
  return FF_OK;
}

extern "C" int ff_loss_ssim(const float* sr, const float* hr, int B, int H, int W, const float* gauss11, float weight, float* dsr,
                            int accumulate, float* value, float* work, long long work_floats, void* stream) {
  const int comp = LS_SSIM;
  LS_ARGS_OK("ff_loss_ssim");
  FF_CHECK_ARG(gauss11 && B * 3 <= 65535, "ff_loss_ssim: bad args");
  const long long n = (long long)B * H * W * 3;
  const dim3 grid(ff_cdiv(W, LS_T), ff_cdiv(H, LS_T), B * 3);
  const int nparts = (int)(grid.x * grid.y * grid.z);
  float* coef = work;
  float* part = work + 3 * n;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ssim_fwd_kernel, grid, dim3(256), 0, st, sr, hr, H, W, gauss11, dsr ? coef : (float*)nullptr, part);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, part, nparts, -1.0f / (float)n, 1.0f, value);
  if (dsr) hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(256), 0, st, sr, hr, H, W, gauss11, coef, weight / (float)n, dsr, accumulate);
  FF_LAUNCH_CHECK("ff_loss_ssim");
  return FF_OK;
}

extern "C" int ff_loss_edge(const float* sr, const float* hr, int B, int H, int W, float weight, float* dsr, int accumulate, float* value,
                            float* work, long long work_floats, void* stream) {
  const int comp = LS_EDGE;
  LS_ARGS_OK("ff_loss_edge");
  const long long n = (long long)B * H * W * 3;
  const int nb = ls_blocks(n);
  float* sgn = work;
  float* part = work + 2 * n;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(edge_fwd_kernel, dim3(nb), dim3(256), 0, st, sr, hr, B, H, W, dsr ? sgn : (float*)nullptr, part);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, part, nb, 1.0f / (float)n, 0.f, value);
  if (dsr) hipLaunchKernelGGL(edge_bwd_kernel, dim3(nb), dim3(256), 0, st, sr, B, H, W, sgn, weight / (float)n, dsr, accumulate);
  FF_LAUNCH_CHECK("ff_loss_edge");
  return FF_OK;
}

extern "C" int ff_loss_swt(const float* sr, const float* hr, int B, int H, int W, float weight, float* dsr, int accumulate, float* value,
                           float* work, long long work_floats, void* stream) {
  const int comp = LS_SWT;
  LS_ARGS_OK("ff_loss_swt");
  FF_CHECK_ARG(H > 2 && W > 2, "ff_loss_swt: level 2 reflect-pads by 2, so H and W must exceed 2");
  const long long n = (long long)B * H * W * 3;
  const int nb = ls_blocks(n);
  float* cA = work;                                       // [2][n]: cA0 of the prediction, of the target
  float* s0 = work + 2 * n;                               // [4][n]
  float* s1 = work + 6 * n;                               // [4][n]
  float* part = work + 10 * n;                            // [2][LS_NB]
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(swt_l0_kernel, dim3(nb), dim3(256), 0, st, sr, hr, B, H, W, cA, dsr ? s0 : (float*)nullptr, part);
  hipLaunchKernelGGL(swt_l1_kernel, dim3(nb), dim3(256), 0, st, cA, B, H, W, dsr ? s1 : (float*)nullptr, part + nb);
  // both levels' partials are contiguous: [0, nb) level 0, [nb, 2 nb) level 1
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, part, 2 * nb, 1.0f / (2.0f * (float)n), 0.f, value);
  if (dsr) {
    hipLaunchKernelGGL(swt_adj1_kernel, dim3(nb), dim3(256), 0, st, s1, B, H, W, s0);
    hipLaunchKernelGGL(swt_adj0_kernel, dim3(nb), dim3(256), 0, st, sr, s0, B, H, W, weight / (2.0f * (float)n), dsr, accumulate);
  }
  FF_LAUNCH_CHECK("ff_loss_swt");
  return FF_OK;
}

extern "C" int ff_loss_fft(const float* sr, const float* hr, int B, int H, int W, const float* twW_cos, const float* twW_sin,
                           const float* twH_cos, const float* twH_sin, float weight, float* dsr, int accumulate, float* value, float* work,
                           long long work_floats, void* stream) {
  const int comp = LS_FFT;
  LS_ARGS_OK("ff_loss_fft");
  FF_CHECK_ARG(twW_cos && twW_sin && twH_cos && twH_sin && H > 1 && W > 1, "ff_loss_fft: bad args");
  const long long n = (long long)B * H * W * 3, spec = (long long)B * 3 * H * (W / 2 + 1) * 2;
  const int planes = B * 3, HW = H * W;
  float* P = work;
  float* T = work + n;
  float* SP = work + 2 * n;
  float* ST = SP + spec;
  float* dft = ST + spec;
  float* part = dft + spec;
  hipStream_t st = (hipStream_t)stream;
  const int nb = ls_blocks(n);
  hipLaunchKernelGGL(nhwc_to_planes_kernel, dim3(nb), dim3(256), 0, st, sr, hr, n, HW, P, T);
  FF_LAUNCH_CHECK("ff_loss_fft");
  if (int rc = ff_rfft2(P, planes, H, W, twW_cos, twW_sin, twH_cos, twH_sin, dft, spec, SP, stream)) return rc;
  if (int rc = ff_rfft2(T, planes, H, W, twW_cos, twW_sin, twH_cos, twH_sin, dft, spec, ST, stream)) return rc;
  const int cy = H / 2, cx = W / 2;
  const float maxd = (float)sqrt((double)cy * cy + (double)cx * cx);
  const int nbs = ls_blocks(spec / 2);
  hipLaunchKernelGGL(fft_loss_kernel, dim3(nbs), dim3(256), 0, st, SP, ST, planes, H, W, maxd, weight / (float)n, dsr ? 1 : 0, part);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, part, nbs, 1.0f / (float)n, 0.f, value);
  FF_LAUNCH_CHECK("ff_loss_fft");
  if (dsr) {
    if (int rc = ff_irfft2(SP, planes, H, W, twW_cos, twW_sin, twH_cos, twH_sin, dft, spec, P, stream)) return rc;
    hipLaunchKernelGGL(planes_to_nhwc_grad_kernel, dim3(nb), dim3(256), 0, st, sr, P, n, HW, dsr, accumulate);
    FF_LAUNCH_CHECK("ff_loss_fft");
  }
  return FF_OK;
}

// total[0] = sum_k weights[k] * values[k], k in order, one fp32 add at a time (the reference's `total_loss = total_loss + w * l`)
__global__ void loss_combine_kernel(const float* __restrict__ values, const float* __restrict__ weights, int k, float* __restrict__ total) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float t = 0.f;
  for (int i = 0; i < k; ++i) t = t + weights[i] * values[i];
  total[0] = t;
}

extern "C" int ff_loss_combine(const float* values, const float* weights, int k, float* total, void* stream) {
  FF_CHECK_ARG(values && weights && total && k > 0, "ff_loss_combine: bad args");
  hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, values, weights, k, total);
  FF_LAUNCH_CHECK("ff_loss_combine");
  return FF_OK;
}
