// c2r along W of one spectrum row: stage the row and the twiddles in LDS, then one output sample per thread and step as two
// interleaved partial sums.  Shared as text by irdft_rows_bands_body and irdft_rows_kernel (freq.hip includes this file twice).
// Expects sm (urow[Wf][2] | cos[W] | sin[W]), U, r, W, Wf, tc, ts and IRDFT_ROW_STORE, the including kernel's statements for
// sample w (they read w, s0, s1 and nrm; the sample is (s0 + s1) * nrm).
  float* urow = sm; float* cs = sm + irdft_off_cos_f(Wf); float* sn = cs + W;      // sn at irdft_off_sin_f(Wf, W), written over cs: from sm the kernels' scalar registers moved
  for (int i = threadIdx.x; i < 2 * Wf; i += 256) urow[i] = U[(long long)r * Wf * 2 + i];
  for (int i = threadIdx.x; i < W; i += 256) { cs[i] = tc[i]; sn[i] = ts[i]; }
  __syncthreads();
  const float nrm = 1.0f / sqrtf((float)W);
  const int kmax = (W - 1) / 2;                           // bins with a conjugate partner
  for (int w = threadIdx.x; w < W; w += 256) {
    float s0 = urow[0], s1 = 0.f;
    if ((W & 1) == 0) s0 += ((w & 1) ? -1.f : 1.f) * urow[2 * (W / 2)];
    int idx = 0, k = 1;
    for (; k + 1 <= kmax; k += 2) {
      idx += w;
      if (idx >= W) idx -= W;
      s0 += 2.f * (urow[2 * k] * cs[idx] - urow[2 * k + 1] * sn[idx]);
      idx += w;
      if (idx >= W) idx -= W;
      s1 += 2.f * (urow[2 * k + 2] * cs[idx] - urow[2 * k + 3] * sn[idx]);
    }
    for (; k <= kmax; ++k) {
      idx += w;
      if (idx >= W) idx -= W;
      s0 += 2.f * (urow[2 * k] * cs[idx] - urow[2 * k + 1] * sn[idx]);
    }
    IRDFT_ROW_STORE
  }
