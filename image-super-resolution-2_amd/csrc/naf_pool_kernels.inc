// ff_dwconv3_gate_pool's two kernels (naf_fused.hip includes this file twice).  NP_DW_KERNEL / NP_REDUCE_KERNEL name them; NP_IMAGES = 0 are
// the single-image forms, NP_IMAGES = 1 the forms for B images in one launch with the image in blockIdx.y: blockIdx.x and gridDim.x are
// what ONE image's launch has, so every image keeps its item-to-workgroup assignment and the order of every sum.
__global__ __launch_bounds__(256) void NP_DW_KERNEL(const float* __restrict__ in, int ldi, float* __restrict__ out, int ldo,
                                                                int H, int W, int C, const float* __restrict__ w, const float* __restrict__ bias,
                                                                float* __restrict__ part) {
  extern __shared__ float4 red[];                      // [ppb][C/4]: pool4_lds
#if NP_IMAGES
  {                                                    // image blockIdx.y: its pixels, and its rows of part [B][gridDim.x][C]
    const long long P = (long long)H * W, b = blockIdx.y;
    in += b * P * ldi;
    out += b * P * ldo;
    part += b * gridDim.x * C;
  }
#endif
  const int cv = C >> 2, ppb = 256 / cv;               // float4 channel groups, (column, strip) items per block iteration
  const int cg = threadIdx.x % cv, ps = threadIdx.x / cv;
  const int nstrip = (H + 3) >> 2;
  const long long items = (long long)nstrip * W;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc_sum = z4;
  if (ps < ppb) {
    const int c = 4 * cg;
    for (long long it = (long long)blockIdx.x * ppb + ps; it < items; it += (long long)gridDim.x * ppb) {
      const int x = (int)(it % W), y0 = (int)(it / W) * 4;
      f32x4 ga[4];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int ch = c + half * C;
        f32x4 wt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wt[k] = *reinterpret_cast<const f32x4*>(w + k * 2 * C + ch);
        const f32x4 bs = *reinterpret_cast<const f32x4*>(bias + ch);
        f32x4 win[6][3];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          const int iy = y0 - 1 + r;
          const bool oky = (unsigned)iy < (unsigned)H;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const int ix = x - 1 + k;
            const bool ok = oky && (unsigned)ix < (unsigned)W;
            const f32x4 u = *reinterpret_cast<const f32x4*>(in + (ok ? ((long long)iy * W + ix) * ldi + ch : 0));
            win[r][k] = ok ? u : z4;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          f32x4 a = bs;
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) a += win[r + ky][kx] * wt[ky * 3 + kx];
          ga[r] = half == 0 ? a : ga[r] * a;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (y0 + r < H) {
          *reinterpret_cast<f32x4*>(out + ((long long)(y0 + r) * W + x) * ldo + c) = ga[r];
          acc_sum += ga[r];
        }
    }
    red[ps * cv + cg] = (float4){acc_sum[0], acc_sum[1], acc_sum[2], acc_sum[3]};
  }
  __syncthreads();
  if (ps == 0) {
    float4 s = red[cg];
    for (int r = 1; r < ppb; ++r) { const float4 t = red[r * cv + cg]; s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w; }
    *reinterpret_cast<float4*>(part + (long long)blockIdx.x * C + 4 * cg) = s;
  }
}

// sum of the per-workgroup partials: 16 channels x 16 partial-lanes per workgroup, 4 independent accumulators per thread
__global__ __launch_bounds__(256) void NP_REDUCE_KERNEL(const float* __restrict__ part, int nch, int C, float invP, float* __restrict__ out) {
  __shared__ float red[16][17];
#if NP_IMAGES
  part += (long long)blockIdx.y * nch * C;             // image blockIdx.y: part [B][nch][C] -> out [B][C]
  out += (long long)blockIdx.y * C;
#endif
  const int cl = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (c < C) {
    int i = r;
    for (; i + 48 < nch; i += 64) {
      s0 += part[(long long)i * C + c];
      s1 += part[(long long)(i + 16) * C + c];
      s2 += part[(long long)(i + 32) * C + c];
      s3 += part[(long long)(i + 48) * C + c];
    }
    for (; i < nch; i += 16) s0 += part[(long long)i * C + c];
  }
  red[r][cl] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (r == 0 && c < C) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k][cl];
    out[c] = s * invP;
  }
}
