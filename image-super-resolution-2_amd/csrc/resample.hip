// Resamplers with PyTorch's exact index/weight conventions (ATen UpSample.h):
//   bilinear, align_corners=False:  src = max(scale*(dst+0.5)-0.5, 0); i0 = min(floor(src), n-1); i1 = min(i0+1, n-1)
//   bicubic,  align_corners=False:  src = scale*(dst+0.5)-0.5 (not clamped), A = -0.75, border-clamped taps
//   scale = 1/scale_factor when the caller passed scale_factor (nafnet/__init__.py:128-133 x4 bicubic,
//   fusion_network.py:590,595 x0.5 / x0.25), else in/out (every F.interpolate(size=...) site:
//   hierarchical_fusion.py:147-181, enhanced_fusion.py:550,620,640,675, edge_enhancement.py:203,245,
//   multi_domain_frequency.py:296,366).  The host computes `scale` exactly as ATen does and passes it.
// Generic element strides on both sides let one kernel serve planar (NCHW) and NHWC tensors and write
// straight into a channel slice of a wider NHWC tensor.  HBM-bound.
#include "ff_common.h"

struct ResizeParams {
  const float* in; float* out;
  long long isb, isc, isy, isx, osb, osc, osy, osx;
  int B, C, Hi, Wi, Ho, Wo;
  float sh, sw;
  int mode;
  float mul;
};

__device__ __forceinline__ void cubic_coeffs(float t, float w[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x3 = 2.f - t, u = 1.f - t;
  w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  w[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

__global__ __launch_bounds__(256) void resize_kernel(ResizeParams p) {
  const long long total = (long long)p.B * p.Ho * p.Wo * p.C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    int c, x, y, b;
    if (p.osc == 1) {        // channel fastest (NHWC out)
      c = (int)(i % p.C); long long t = i / p.C;
      x = (int)(t % p.Wo); t /= p.Wo;
      y = (int)(t % p.Ho); b = (int)(t / p.Ho);
    } else {                 // x fastest (planar out)
      x = (int)(i % p.Wo); long long t = i / p.Wo;
      y = (int)(t % p.Ho); t /= p.Ho;
      c = (int)(t % p.C); b = (int)(t / p.C);
    }
    const float* src = p.in + b * p.isb + c * p.isc;
    float v;
    if (p.mode == 0) {
      int y0, y1, x0, x1; float ly, lx;
      if (p.Ho == p.Hi) { y0 = y1 = y; ly = 0.f; }
      else {
        float sy = fmaxf(p.sh * ((float)y + 0.5f) - 0.5f, 0.f);
        y0 = min((int)floorf(sy), p.Hi - 1); y1 = min(y0 + 1, p.Hi - 1);
        ly = fminf(fmaxf(sy - (float)y0, 0.f), 1.f);
      }
      if (p.Wo == p.Wi) { x0 = x1 = x; lx = 0.f; }
      else {
        float sx = fmaxf(p.sw * ((float)x + 0.5f) - 0.5f, 0.f);
        x0 = min((int)floorf(sx), p.Wi - 1); x1 = min(x0 + 1, p.Wi - 1);
        lx = fminf(fmaxf(sx - (float)x0, 0.f), 1.f);
      }
      const float a = src[y0 * p.isy + x0 * p.isx], bq = src[y0 * p.isy + x1 * p.isx];
      const float cq = src[y1 * p.isy + x0 * p.isx], d = src[y1 * p.isy + x1 * p.isx];
      v = (1.f - ly) * ((1.f - lx) * a + lx * bq) + ly * ((1.f - lx) * cq + lx * d);
    } else {
      const float sy = p.sh * ((float)y + 0.5f) - 0.5f, sx = p.sw * ((float)x + 0.5f) - 0.5f;
      const int iy = (int)floorf(sy), ix = (int)floorf(sx);
      float wy[4], wx[4];
      cubic_coeffs(sy - (float)iy, wy);
      cubic_coeffs(sx - (float)ix, wx);
      v = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int yy = min(max(iy - 1 + j, 0), p.Hi - 1);
        float r = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int xx = min(max(ix - 1 + k, 0), p.Wi - 1);
          r += wx[k] * src[yy * p.isy + xx * p.isx];
        }
        v += wy[j] * r;
      }
    }
    p.out[b * p.osb + c * p.osc + y * p.osy + x * p.osx] = v * p.mul;
  }
}

// Bilinear, channel-last on both sides, four channels per thread: the index / weight arithmetic is shared by a float4 and every
// access is 16 bytes (the generic kernel above moves one float per thread: ~1 TB/s on the 64-channel up-samplings of the
// hierarchical fusion, hierarchical_fusion.py:147-181).
__global__ __launch_bounds__(256) void resize_bilinear_nhwc4_kernel(ResizeParams p) {
  const int c4n = p.C >> 2;
  const long long total = (long long)p.B * p.Ho * p.Wo * c4n;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % c4n) * 4; long long t = i / c4n;
    const int x = (int)(t % p.Wo); t /= p.Wo;
    const int y = (int)(t % p.Ho); const int b = (int)(t / p.Ho);
    int y0, y1, x0, x1; float ly, lx;
    if (p.Ho == p.Hi) { y0 = y1 = y; ly = 0.f; }
    else {
      const float sy = fmaxf(p.sh * ((float)y + 0.5f) - 0.5f, 0.f);
      y0 = min((int)floorf(sy), p.Hi - 1); y1 = min(y0 + 1, p.Hi - 1);
      ly = fminf(fmaxf(sy - (float)y0, 0.f), 1.f);
    }
    if (p.Wo == p.Wi) { x0 = x1 = x; lx = 0.f; }
    else {
      const float sx = fmaxf(p.sw * ((float)x + 0.5f) - 0.5f, 0.f);
      x0 = min((int)floorf(sx), p.Wi - 1); x1 = min(x0 + 1, p.Wi - 1);
      lx = fminf(fmaxf(sx - (float)x0, 0.f), 1.f);
    }
    const float* src = p.in + b * p.isb + c;
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + y0 * p.isy + x0 * p.isx), bq = *reinterpret_cast<const f32x4*>(src + y0 * p.isy + x1 * p.isx);
    const f32x4 cq = *reinterpret_cast<const f32x4*>(src + y1 * p.isy + x0 * p.isx), d = *reinterpret_cast<const f32x4*>(src + y1 * p.isy + x1 * p.isx);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e)            // same association as the scalar kernel: bit-identical results
      v[e] = ((1.f - ly) * ((1.f - lx) * a[e] + lx * bq[e]) + ly * ((1.f - lx) * cq[e] + lx * d[e])) * p.mul;
    *reinterpret_cast<f32x4*>(p.out + b * p.osb + c + y * p.osy + x * p.osx) = v;
  }
}

extern "C" int ff_resize(const float* in, long long isb, long long isc, long long isy, long long isx, int Hi, int Wi,
                         float* out, long long osb, long long osc, long long osy, long long osx, int Ho, int Wo, int B,
                         int C, float scale_h, float scale_w, int mode, float mul, void* stream) {
  FF_CHECK_ARG(in && out && B > 0 && C > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "ff_resize: bad args");
  FF_CHECK_ARG(mode == 0 || mode == 1, "ff_resize: mode must be 0 (bilinear) or 1 (bicubic)");
  ResizeParams p;
  p.in = in; p.out = out; p.isb = isb; p.isc = isc; p.isy = isy; p.isx = isx;
  p.osb = osb; p.osc = osc; p.osy = osy; p.osx = osx;
  p.B = B; p.C = C; p.Hi = Hi; p.Wi = Wi; p.Ho = Ho; p.Wo = Wo; p.sh = scale_h; p.sw = scale_w; p.mode = mode; p.mul = mul;
  const bool v4 = mode == 0 && isc == 1 && osc == 1 && C % 4 == 0 && isx % 4 == 0 && isy % 4 == 0 && isb % 4 == 0 && osx % 4 == 0 && osy % 4 == 0 &&
                  osb % 4 == 0 && (((uintptr_t)in) & 15) == 0 && (((uintptr_t)out) & 15) == 0;
  long long nb = ((long long)B * Ho * Wo * (v4 ? C / 4 : C) + 255) / 256;
  if (nb > 16384) nb = 16384;
  if (v4) hipLaunchKernelGGL(resize_bilinear_nhwc4_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(resize_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, p);
  FF_LAUNCH_CHECK("ff_resize");
  return FF_OK;
}

// 2x2 average pool, stride 2, NHWC (edge_enhancement.py:202)
__global__ __launch_bounds__(256) void avgpool2_kernel(const float* __restrict__ in, int ldi, float* __restrict__ out, int ldo,
                                                       int B, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2;
  const long long total = (long long)B * Ho * Wo * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C); long long t = i / C;
    const int x = (int)(t % Wo); t /= Wo;
    const int y = (int)(t % Ho); const int b = (int)(t / Ho);
    const float* s = in + (((long long)b * H + 2 * y) * W + 2 * x) * ldi + c;
    out[(((long long)b * Ho + y) * Wo + x) * ldo + c] = (s[0] + s[ldi] + s[(long long)W * ldi] + s[(long long)(W + 1) * ldi]) * 0.25f;
  }
}

extern "C" int ff_avgpool2(const float* in, int ldi, float* out, int ldo, int B, int H, int W, int C, void* stream) {
  FF_CHECK_ARG(in && out && B > 0 && H >= 2 && W >= 2 && C > 0 && ldi >= C && ldo >= C, "ff_avgpool2: bad args");
  long long nb = ((long long)B * (H / 2) * (W / 2) * C + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(avgpool2_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, in, ldi, out, ldo, B, H, W, C);
  FF_LAUNCH_CHECK("ff_avgpool2");
  return FF_OK;
}

// ---- cached-expert training sets (isr2_amd.cache.build_from_folders) -------------------------------------------------------------
// Aligned LR / HR patch pairs cut out of the uploaded uint8 images: lr_u8 [h][w][3], hr_u8 [4h][4w][3] -> lr_out [K][3][p][p],
// hr_out [K][3][4p][4p], value = u8 / 255 (IEEE division, as u8hwc_to_f32nchw_kernel).  Patch k starts at LR (top, left) =
// pos[k] and at HR (4 top, 4 left).  One work item = four consecutive pixels of one patch row: twelve byte loads (a pixel is three
// bytes, so the address is unaligned whenever `left` is odd -- bytes have no alignment) and one 16-byte store into each of the three
// planes, so a wave writes whole row segments.  VEC = false (p % 4 != 0 on the LR side, or an unaligned output): scalar stores.
// Items [0, n_lr) cut the LR patches, the rest the HR patches.  The positions are the caller's contract (ops.crop_pairs_u8 checks
// them on the host before the launch); they are clamped here all the same, so no table can make the kernel leave the images.
template <bool VEC>
__device__ __forceinline__ void crop_item(const unsigned char* __restrict__ img, int H, int W, int top, int left, int P, int q, long long item,
                                          float* __restrict__ out) {
  const int xg = (int)(item % q); long long t = item / q;
  const int y = (int)(t % P); const int k = (int)(t / P);
  const int x = xg * 4;
  const unsigned char* src = img + ((long long)(top + y) * W + left + x) * 3;
  float* dst = out + ((long long)k * 3 * P + y) * P + x;
  const long long plane = (long long)P * P;
  if (VEC) {
    f32x4 v[3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][j] = __fdiv_rn((float)src[j * 3 + c], 255.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(dst + c * plane) = v[c];
  } else {
    const int n = min(4, P - x);
    for (int j = 0; j < n; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[c * plane + j] = __fdiv_rn((float)src[j * 3 + c], 255.0f);
  }
}

template <bool VEC_LR, bool VEC_HR>
__global__ __launch_bounds__(256) void crop_pairs_u8_kernel(const unsigned char* __restrict__ lr, const unsigned char* __restrict__ hr, int h, int w,
                                                            const int* __restrict__ pos, int K, int p, float* __restrict__ lr_out,
                                                            float* __restrict__ hr_out) {
  const int q_lr = (p + 3) >> 2, q_hr = p;                       // four-pixel groups per patch row
  const long long n_lr = (long long)K * p * q_lr, total = n_lr + (long long)K * 4 * p * q_hr;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const bool is_hr = i >= n_lr;
    const long long item = is_hr ? i - n_lr : i;
    const int k = (int)(item / (is_hr ? (long long)4 * p * q_hr : (long long)p * q_lr));
    const int top = min(max(pos[2 * k], 0), h - p), left = min(max(pos[2 * k + 1], 0), w - p);
    if (is_hr) crop_item<VEC_HR>(hr, 4 * h, 4 * w, 4 * top, 4 * left, 4 * p, q_hr, item, hr_out);
    else crop_item<VEC_LR>(lr, h, w, top, left, p, q_lr, item, lr_out);
  }
}

extern "C" int ff_crop_pairs_u8(const unsigned char* lr_u8, const unsigned char* hr_u8, int h, int w, const int* pos, int K, int p,
                                float* lr_out, float* hr_out, void* stream) {
  FF_CHECK_ARG(lr_u8 && hr_u8 && pos && lr_out && hr_out, "ff_crop_pairs_u8: null pointer");
  FF_CHECK_ARG(K >= 1 && p >= 1 && h >= 1 && w >= 1, "ff_crop_pairs_u8: bad sizes (K %d, p %d, image %d x %d)", K, p, h, w);
  FF_CHECK_ARG(p <= h && p <= w, "ff_crop_pairs_u8: a %d x %d patch does not fit the %d x %d image", p, p, h, w);
  FF_CHECK_ARG(h <= (1 << 20) && w <= (1 << 20) && p <= 8192 && K <= (1 << 20), "ff_crop_pairs_u8: sizes out of range");
  const bool vec_hr = (((uintptr_t)hr_out) & 15) == 0, vec_lr = p % 4 == 0 && (((uintptr_t)lr_out) & 15) == 0;
  const long long total = (long long)K * p * ((p + 3) / 4 + 4 * (long long)p);
  long long nb = (total + 255) / 256;
  if (nb > 8192) nb = 8192;
#define FF_CROP_LAUNCH(A, B) \
  hipLaunchKernelGGL((crop_pairs_u8_kernel<A, B>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, lr_u8, hr_u8, h, w, pos, K, p, lr_out, hr_out)
  if (vec_lr && vec_hr) FF_CROP_LAUNCH(true, true);
  else if (vec_hr) FF_CROP_LAUNCH(false, true);
  else FF_CROP_LAUNCH(false, false);
#undef FF_CROP_LAUNCH
  FF_LAUNCH_CHECK("ff_crop_pairs_u8");
  return FF_OK;
}

// Antialiased bicubic x1/4 (the degradation the x4 track is defined on; F.interpolate(mode='bicubic', antialias=True,
// align_corners=False)), planar fp32 [planes][Hi][Wi] -> [planes][Ho][Wo] with Hi = 4 Ho, Wi = 4 Wo.  Separable, horizontal pass
// first.  Each axis is driven by a host table (ops.aa_tables): span [O][2] = (first input index, taps <= 16) and wt [O][16] =
// the normalised fp32 weights, zero padded.  Both passes accumulate acc = fma(w_j, x[first + j], acc) from acc = 0 in ascending j.
// One workgroup per 16 x 64 output tile: the horizontal pass of the tile's input rows (at most 4*16 + 16) goes to LDS -- a thread
// keeps one output column and its 16 weights in registers and walks down the rows --, the vertical pass reads LDS columns (lanes on
// consecutive banks) with wave-uniform weights and stores 64-float row segments.  Table entries are clamped to the image and to
// the staged rows, so a wrong table gives wrong values, never an access outside the buffers.
#define AA_TAPS 16
#define AA_TOY 16
#define AA_TOX 64
#define AA_ROWS (4 * AA_TOY + AA_TAPS)

__global__ __launch_bounds__(256) void resize_aa_kernel(const float* __restrict__ in, float* __restrict__ out, int Hi, int Wi, int Ho, int Wo,
                                                        const int* __restrict__ span_w, const float* __restrict__ wt_w,
                                                        const int* __restrict__ span_h, const float* __restrict__ wt_h) {
  __shared__ float rows[AA_ROWS][AA_TOX];
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int ox = blockIdx.x * AA_TOX + lx, oy0 = blockIdx.y * AA_TOY;
  const int oy1 = min(oy0 + AA_TOY, Ho) - 1;                     // last output row of the tile
  const float* src = in + (long long)blockIdx.z * Hi * Wi;
  // input rows [r0, r0 + nr) cover every tap of the tile's output rows
  const int c0 = min(max(span_h[2 * oy0 + 1], 0), min(AA_TAPS, Hi));
  const int r0 = min(max(span_h[2 * oy0], 0), Hi - c0);
  const int c1 = min(max(span_h[2 * oy1 + 1], 0), min(AA_TAPS, Hi));
  const int nr = min(min(max(span_h[2 * oy1], 0), Hi - c1) + c1 - r0, min(AA_ROWS, Hi - r0));
  if (ox < Wo) {
    const int cnt = min(max(span_w[2 * ox + 1], 0), min(AA_TAPS, Wi));
    const int x0 = min(max(span_w[2 * ox], 0), Wi - cnt);
    float w[AA_TAPS];
#pragma unroll
    for (int j = 0; j < AA_TAPS; j += 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(wt_w + (long long)ox * AA_TAPS + j);
      w[j] = t[0]; w[j + 1] = t[1]; w[j + 2] = t[2]; w[j + 3] = t[3];
    }
    for (int r = ly; r < nr; r += 4) {
      const float* line = src + (long long)(r0 + r) * Wi + x0;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < AA_TAPS; ++j)
        if (j < cnt) acc = fmaf(w[j], line[j], acc);
      rows[r][lx] = acc;
    }
  }
  __syncthreads();
  if (ox >= Wo) return;
  for (int oy = oy0 + ly; oy <= oy1; oy += 4) {                  // one wave = one output row: span and weights are wave-uniform
    const int cnt = min(max(span_h[2 * oy + 1], 0), min(AA_TAPS, Hi));
    const int y0 = min(max(span_h[2 * oy], 0), Hi - cnt) - r0;
    const float* wy = wt_h + (long long)oy * AA_TAPS;
    float acc = 0.f;
    for (int j = 0; j < cnt; ++j) {
      const int r = y0 + j;
      if (r >= 0 && r < nr) acc = fmaf(wy[j], rows[r][lx], acc);
    }
    out[((long long)blockIdx.z * Ho + oy) * Wo + ox] = acc;
  }
}

extern "C" int ff_resize_aa(const float* in, float* out, int planes, int Hi, int Wi, int Ho, int Wo, const int* span_w, const float* wt_w,
                            const int* span_h, const float* wt_h, void* stream) {
  FF_CHECK_ARG(in && out && span_w && wt_w && span_h && wt_h, "ff_resize_aa: null pointer");
  FF_CHECK_ARG(planes >= 1 && planes <= 65535 && Ho >= 1 && Wo >= 1, "ff_resize_aa: bad sizes (planes %d, out %d x %d)", planes, Ho, Wo);
  FF_CHECK_ARG(Ho <= (1 << 20) && Wo <= (1 << 20) && Hi == 4 * Ho && Wi == 4 * Wo,
               "ff_resize_aa: the input must be exactly 4x the output, got %d x %d -> %d x %d", Hi, Wi, Ho, Wo);
  FF_CHECK_ARG((((uintptr_t)wt_w) & 15) == 0, "ff_resize_aa: wt_w must be 16-byte aligned");
  const dim3 grid((unsigned)((Wo + AA_TOX - 1) / AA_TOX), (unsigned)((Ho + AA_TOY - 1) / AA_TOY), (unsigned)planes);
  FF_CHECK_ARG(grid.y <= 65535, "ff_resize_aa: output too tall (%d rows)", Ho);
  hipLaunchKernelGGL(resize_aa_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, out, Hi, Wi, Ho, Wo, span_w, wt_w, span_h, wt_h);
  FF_LAUNCH_CHECK("ff_resize_aa");
  return FF_OK;
}

// ---- OpenCV's INTER_CUBIC restated (isr2_amd.epoch.live_val_images: the reference's ValidationDataset, dataset.py:473-506) ------------
// cv2.resize(..., interpolation=INTER_CUBIC) of planar fp32 [planes][Hi][Wi] -> [planes][Ho][Wo] at any ratio, up or down: four taps per
// axis whatever the ratio (no antialiasing when shrinking), replicated border, no clamping of values.  Each axis is driven by a host table
// (ops.cv_cubic_tables): idx [O][4] int32 = the taps s - 1 .. s + 2 clamped to the image, wt [O][4] fp32 = interpolateCubic's weights
// (A = -0.75) of x = f - s, f = float((d + 0.5) * scale - 0.5), s = floor(f).  Fixed arithmetic, so that a numpy restatement
// (tests/golden/cv_cubic_ref.py) matches bit for bit: per source row h = ((v0 a0 + v1 a1) + v2 a2) + v3 a3, then
// out = ((h0 b0 + h1 b1) + h2 b2) + h3 b3, every product and every sum rounded on its own -- contraction is OFF in cvc_dot4 (a fused
// multiply-add would change the bits; the rest of this file keeps the compiler's default).  A gather that runs once per validation image:
// direct form, no LDS.  One work item = up to four consecutive output pixels of one row; VEC (Wo % 4 == 0 and a 16-byte aligned output):
// one 16-byte store, else scalar stores.  Table indices are clamped again here, so a wrong table gives wrong values, never an access
// outside the buffers.  Offsets are 64-bit.
__device__ __forceinline__ float cvc_dot4(float v0, float v1, float v2, float v3, float w0, float w1, float w2, float w3) {
#pragma clang fp contract(off)
  const float p0 = v0 * w0, p1 = v1 * w1, p2 = v2 * w2, p3 = v3 * w3;
  return ((p0 + p1) + p2) + p3;
}

template <bool VEC>
__global__ __launch_bounds__(256) void resize_cv_cubic_kernel(const float* __restrict__ in, float* __restrict__ out, int planes, int Hi, int Wi,
                                                              int Ho, int Wo, const int* __restrict__ idx_w, const float* __restrict__ wt_w,
                                                              const int* __restrict__ idx_h, const float* __restrict__ wt_h) {
  const int q = (Wo + 3) >> 2;                                   // four-pixel groups per output row
  const long long total = (long long)planes * Ho * q;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int xg = (int)(i % q); long long t = i / q;
    const int oy = (int)(t % Ho); const long long pl = t / Ho;
    const float* src = in + pl * Hi * Wi;
    const float* line[4]; float b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      line[j] = src + (long long)min(max(idx_h[4ll * oy + j], 0), Hi - 1) * Wi;
      b[j] = wt_h[4ll * oy + j];
    }
    const int x0 = xg * 4, n = VEC ? 4 : min(4, Wo - x0);
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < n) {
        const long long tw = 4ll * (x0 + e);
        int cx[4]; float a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          cx[k] = min(max(idx_w[tw + k], 0), Wi - 1);
          a[k] = wt_w[tw + k];
        }
        float h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = cvc_dot4(line[j][cx[0]], line[j][cx[1]], line[j][cx[2]], line[j][cx[3]], a[0], a[1], a[2], a[3]);
        r[e] = cvc_dot4(h[0], h[1], h[2], h[3], b[0], b[1], b[2], b[3]);
      }
    }
    float* dst = out + (pl * Ho + oy) * Wo + x0;
    if (VEC) *reinterpret_cast<f32x4*>(dst) = r;
    else
      for (int e = 0; e < n; ++e) dst[e] = r[e];
  }
}

extern "C" int ff_resize_cv_cubic(const float* in, float* out, int planes, int Hi, int Wi, int Ho, int Wo, const int* idx_w, const float* wt_w,
                                  const int* idx_h, const float* wt_h, void* stream) {
  FF_CHECK_ARG(in && out && idx_w && wt_w && idx_h && wt_h, "ff_resize_cv_cubic: null pointer");
  FF_CHECK_ARG(planes >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1, "ff_resize_cv_cubic: bad sizes (planes %d, %d x %d -> %d x %d)", planes,
               Hi, Wi, Ho, Wo);
  FF_CHECK_ARG(planes <= (1 << 20) && Hi <= (1 << 20) && Wi <= (1 << 20) && Ho <= (1 << 20) && Wo <= (1 << 20),
               "ff_resize_cv_cubic: sizes out of range (planes %d, %d x %d -> %d x %d)", planes, Hi, Wi, Ho, Wo);
  const long long total = (long long)planes * Ho * ((Wo + 3) / 4);
  long long nb = (total + 255) / 256;                            // grid-stride: the grid is bounded whatever the sizes are
  if (nb > 16384) nb = 16384;
  FF_CHECK_ARG(nb >= 1 && nb <= 16384, "ff_resize_cv_cubic: %lld work items give a grid of %lld blocks", total, nb);
  const bool vec = Wo % 4 == 0 && (((uintptr_t)out) & 15) == 0;
  if (vec) hipLaunchKernelGGL(resize_cv_cubic_kernel<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, in, out, planes, Hi, Wi, Ho, Wo, idx_w, wt_w, idx_h, wt_h);
  else hipLaunchKernelGGL(resize_cv_cubic_kernel<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, in, out, planes, Hi, Wi, Ho, Wo, idx_w, wt_w, idx_h, wt_h);
  FF_LAUNCH_CHECK("ff_resize_cv_cubic");
  return FF_OK;
}
