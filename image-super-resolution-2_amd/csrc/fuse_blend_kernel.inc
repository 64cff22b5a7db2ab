// HR blend kernel of csrc/fusion_ops.hip, one source text for both forms:
//   FB_KERNEL  the kernel's name
//   FB_IMAGES  0: one image;  1: grid (one image's blocks, B), image blockIdx.y of E [B][Hh][Wh][9], hier / out [B][Hh][Wh][3],
//              guide / gates [B][Hl][Wl][3], dif [B][Hl][Wl]
__global__ __launch_bounds__(256) void FB_KERNEL(const float* __restrict__ E, const float* __restrict__ hier,
                                                 const float* __restrict__ guide, const float* __restrict__ gates,
                                                 const float* __restrict__ dif, float* __restrict__ out, int Hh, int Wh,
                                                 int Hl, int Wl) {
#if FB_IMAGES
  {
    const long long ph = (long long)blockIdx.y * Hh * Wh, pl = (long long)blockIdx.y * Hl * Wl;
    E += ph * 9; hier += ph * 3; out += ph * 3; guide += pl * 3; gates += pl * 3; dif += pl;
  }
#endif
  const long long P = (long long)Hh * Wh;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long long)gridDim.x * 256) {
    const int x = (int)(p % Wh), y = (int)(p / Wh);
    int y0, y1, x0, x1; float ly, lx;
    bl_setup(y, Hl, Hh, y0, y1, ly);
    bl_setup(x, Wl, Wh, x0, x1, lx);
    const long long a = (long long)y0 * Wl + x0, b = (long long)y0 * Wl + x1, c = (long long)y1 * Wl + x0, d = (long long)y1 * Wl + x1;
#define BL(T, k, s) ((1.f - ly) * ((1.f - lx) * T[a * s + k] + lx * T[b * s + k]) + ly * ((1.f - lx) * T[c * s + k] + lx * T[d * s + k]))
    float gd[3], gt[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) { gd[e] = BL(guide, e, 3); gt[e] = BL(gates, e, 3); }
    const float df = BL(dif, 0, 1);
#undef BL
    const float gsum = gt[0] + gt[1] + gt[2] + 1e-8f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float eh = E[p * 9 + ch], ed = E[p * 9 + 3 + ch], en = E[p * 9 + 6 + ch];
      const float fw = eh * gd[0] + ed * gd[1] + en * gd[2];
      const float f0 = hier[p * 3 + ch] * 0.7f + fw * 0.3f;
      const float dyn = (eh * gt[0] + ed * gt[1] + en * gt[2]) / gsum;
      out[p * 3 + ch] = f0 * (1.f - 0.3f * df) + dyn * (0.3f * df);
    }
  }
}
