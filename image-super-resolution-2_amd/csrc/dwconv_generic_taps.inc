// Pixel decode and tap loop of the two generic depth-wise kernels (dwconv_vec4_kernel, dwconv_scalar_kernel), shared as text: through a
// decode function or a tap-loop functor the assembly of both moved.  Expects p, idx and the including kernel's DW_CN (channel groups per
// pixel), DW_ACC_INIT (declares its accumulator) and DW_TAP (adds tap (ky, kx) at input pixel (b, iy, ix)); leaves ox, oy, b.
    long long pix = idx / DW_CN;
    const int ox = (int)(pix % p.Wo); pix /= p.Wo;
    const int oy = (int)(pix % p.Ho);
    const int b = (int)(pix / p.Ho);
    DW_ACC_INIT
    for (int ky = 0; ky < p.KH; ++ky) {
      const int iy = oy * p.sy - p.py + ky;
      if ((unsigned)iy >= (unsigned)p.H) continue;
      for (int kx = 0; kx < p.KW; ++kx) {
        const int ix = ox * p.sx - p.px + kx;
        if ((unsigned)ix >= (unsigned)p.W) continue;
        DW_TAP
      }
    }
