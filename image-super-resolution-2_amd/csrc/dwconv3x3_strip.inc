// The 3x3 / stride 1 / pad 1 strip body of dwconv.hip, shared as text by dwconv3x3_strip_kernel and dwconv3x3_ln_strip_kernel (as a
// function over a policy object the register allocation of both moved): a thread owns 4 channels of a 4-row output strip, keeps the 9
// tap weights in registers and slides a 3-column window down 6 input rows, so each output costs 4.5 float4 loads instead of 9 and no
// per-tap weight loads or bounds branches.  One input row at a time (three elements) feeds up to three output rows: the whole 6 x 3
// window never sits in registers next to the nine taps (136 VGPRs -> under 128 = four waves per SIMD for these bandwidth-bound
// kernels); each output still accumulates its taps in (ky, kx) order, so the result is bit-identical to the windowed form.
// Expects p (B, H, W, C, w) and the including kernel's statements
//   DW_STRIP_VECS   the thread's per-channel vectors (they read c and z4),
//   DW_STRIP_TAP    t[k] = the input element at (b, iy, ix), z4 where !ok,
//   DW_STRIP_STORE  the epilogue over acc4[4] (it reads b, y0, ox, c).
  const int c4n = p.C >> 2;
  const int nstrip = (p.H + 3) >> 2;
  const long long total = (long long)p.B * nstrip * p.W * c4n;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const int c = (int)(idx % c4n) * 4;
    long long t = idx / c4n;
    const int ox = (int)(t % p.W); t /= p.W;
    const int y0 = (int)(t % nstrip) * 4;
    const int b = (int)(t / nstrip);
    f32x4 w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = *reinterpret_cast<const f32x4*>(p.w + (long long)k * p.C + c);
    DW_STRIP_VECS
    f32x4 acc4[4] = {z4, z4, z4, z4};
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const int iy = y0 - 1 + r;
      const bool oky = (unsigned)iy < (unsigned)p.H;
      f32x4 t[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int ix = ox - 1 + k;
        const bool ok = oky && (unsigned)ix < (unsigned)p.W;
        DW_STRIP_TAP
      }
#pragma unroll
      for (int ky = 2; ky >= 0; --ky) {                          // output row o = r - ky receives its tap row ky
        const int o = r - ky;
        if (o >= 0 && o < 4) {
          acc4[o] += t[0] * w[ky * 3];
          acc4[o] += t[1] * w[ky * 3 + 1];
          acc4[o] += t[2] * w[ky * 3 + 2];
        }
      }
      asm volatile("" : "+v"(acc4[0]), "+v"(acc4[1]), "+v"(acc4[2]), "+v"(acc4[3]) : : "memory");
    }
    DW_STRIP_STORE
  }
