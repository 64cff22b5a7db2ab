// Window geometry of the windowed-attention kernels: ONE definition of the workgroup -> window decode, the cyclic shift, the
// token index of a window position and the shift-mask region rule.  Plain integer arithmetic that compiles for the device and for
// the host (tests/win_geometry_shim.cpp pins it to a torch.roll / window-partition model).
//
// Coordinates: (y, x) is a position in the SHIFTED, padded grid Hp x Wp (what the window partition cuts); the image is H x W
// (H <= Hp, W <= Wp: DAT pads up to a multiple of the window), (sh, sw) the cyclic shift, (wh, ww) the window.
#pragma once

#if defined(__HIPCC__)
#define FF_HD __host__ __device__ __forceinline__
#else
#define FF_HD inline
#endif

struct FFWinYX { int y, x; };
struct FFWinId { int wx, wy, b; };

// workgroup index -> window column, window row, image (windows are counted x fastest, then y, then the batch)
FF_HD FFWinId ff_win_decode(int bid, int nwx, int nwy) {
  FFWinId w;
  w.wx = bid % nwx; bid /= nwx;
  w.wy = bid % nwy;
  w.b = bid / nwy;
  return w;
}

// Three rules as TEXT, for the sites where a call moves a kernel's registers (attention_bf16.hip's key table, hab_link.hip's tok_of, the
// key tables of attention.hip and ocab_attn.hip); the functions below are written over them, so each rule still has one definition.
// shifted-grid coordinate -> coordinate in the padded image, declared as ints oy, ox: the inverse of torch.roll(-sh, -sw)
// (0 <= sh < Hp, 0 <= sw < Wp)
#define FF_WIN_UNSHIFT_DECL(oy, ox, y, x, sh, sw, Hp, Wp) \
  int oy = (y) + (sh), ox = (x) + (sw);                   \
  if (oy >= (Hp)) oy -= (Hp);                             \
  if (ox >= (Wp)) ox -= (Wp)
// a key window may overhang the grid (OCAB's 24 x 24 keys around a 16 x 16 window): keys outside it are zero keys, not wrapped ones
#define FF_WIN_IN_GRID(y, x, Hp, Wp) ((y) >= 0 && (x) >= 0 && (y) < (Hp) && (x) < (Wp))
// the same test against the image, for a kernel without shift and padding (both bounds of an axis in one unsigned compare)
#define FF_WIN_IN_IMAGE(y, x, H, W) ((unsigned)(y) < (unsigned)(H) && (unsigned)(x) < (unsigned)(W))

FF_HD FFWinYX ff_win_unshift(int y, int x, int sh, int sw, int Hp, int Wp) {
  FF_WIN_UNSHIFT_DECL(oy, ox, y, x, sh, sw, Hp, Wp);
  FFWinYX o;
  o.y = oy; o.x = ox;
  return o;
}

// token index of shifted-grid position (y, x) of image b, -1 where it falls into the padding outside H x W.  (y, x) lies inside
// the grid: the kernels of an overhanging key window test FF_WIN_IN_GRID before they come here
FF_HD int ff_win_token(int b, int y, int x, int sh, int sw, int Hp, int Wp, int H, int W) {
  const FFWinYX o = ff_win_unshift(y, x, sh, sw, Hp, Wp);
  return (o.y < H && o.x < W) ? (b * H + o.y) * W + o.x : -1;
}

// shift-mask region 3 ry + rx of shifted-grid position (y, x): the Swin / HAT mask image, slices (0, -wh), (-wh, -sh), (-sh, end)
// per axis.  Two positions of a window attend to each other only when their regions agree.
FF_HD int ff_win_region(int y, int x, int Hp, int Wp, int wh, int ww, int sh, int sw) {
  const int ry = y < Hp - wh ? 0 : (y < Hp - sh ? 1 : 2);
  const int rx = x < Wp - ww ? 0 : (x < Wp - sw ? 1 : 2);
  return 3 * ry + rx;
}

// only the windows of the last window row / column hold more than one region: everywhere else the mask is all zero
FF_HD bool ff_win_has_regions(int wx, int wy, int nwx, int nwy) { return wy == nwy - 1 || wx == nwx - 1; }
