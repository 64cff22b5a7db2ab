"""numpy restatement of the colour jitter that csrc/color_jitter.hip applies (ops.color_jitter_pairs), the reference's
ColorJitter._apply_jitter (augmentations.py:236-264) with its two OpenCV calls replaced by the published 8-bit definition:

    rgb2hsv8   integer, 12 fractional bits: v = max, d = v - min, S = (d sdiv[v] + 2048) >> 12, H = (h hdiv[d] + 2048) >> 12 (+180 when
               negative; 0..179), h = g - b | b - r + 2d | r - g + 4d by the channel holding v; sdiv[i] = rint(255 * 4096 / i),
               hdiv[i] = rint(180 * 4096 / (6 i)), entry 0 = 0
    hsv2rgb8   fp32: hh = H * (6/180), s = S / 255, vv = V / 255 (products with the fp32 reciprocals), sector = floor(hh), f = hh - sector,
               tab = {vv, vv (1 - s), vv (1 - s f), vv (1 - s (1 - f))}, (b, g, r) = tab[IDX[sector % 6]], byte = rint(255 c) saturated

Every fp32 step is one numpy operation on float32 arrays (no fused multiply-add); the patch mean is defined by exact summation:
mean = float32(float64(bf) * (float64(sum of bytes) / (255.0 * count))).  Whether this equals an OpenCV binary to the last level is
not pinned anywhere (OpenCV is not a dependency): parity unpinned (OpenCV absent)."""
import numpy as np

F = np.float32
_i = np.arange(1, 256, dtype=np.float64)
SDIV = np.concatenate([[0], np.rint(255.0 * 4096.0 / _i)]).astype(np.int64)
HDIV = np.concatenate([[0], np.rint(180.0 * 4096.0 / (6.0 * _i))]).astype(np.int64)
IDX = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def rgb2hsv8(rgb):
    """rgb: integer array [..., 3] of bytes -> (H, S, V) int64 arrays, H in 0..179."""
    q = np.asarray(rgb).astype(np.int64)
    r, g, b = q[..., 0], q[..., 1], q[..., 2]
    v, m = q.max(axis=-1), q.min(axis=-1)
    d = v - m
    s = (d * SDIV[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    hh = (h * HDIV[d] + 2048) >> 12                                    # numpy's >> on int64 is arithmetic
    hh = np.where(hh < 0, hh + 180, hh)
    return hh, s, v


def hsv2rgb8(h, s, v):
    """H, S, V integer arrays -> uint8 [..., 3] (r, g, b)."""
    h, s, v = (np.asarray(a).astype(np.int64) for a in (h, s, v))
    hh = h.astype(F) * (F(6) / F(180))
    sf = s.astype(F) * (F(1) / F(255))
    vv = v.astype(F) * (F(1) / F(255))
    fl = np.floor(hh)
    f = hh - fl
    sec = fl.astype(np.int64) % 6
    one = F(1)
    tab = np.stack([vv, vv * (one - sf), vv * (one - sf * f), vv * (one - sf * (one - f))], axis=-1)       # [..., 4]
    bgr = np.take_along_axis(tab, IDX[sec], axis=-1)                    # [..., 3] = (b, g, r)
    bgr = np.where((s == 0)[..., None], vv[..., None], bgr)
    byte = np.clip(np.rint(bgr * F(255)), 0, 255).astype(np.uint8)
    return byte[..., ::-1]


def saturate8(rgb, sf):
    """The whole saturation step on bytes: uint8 [..., 3] -> uint8 [..., 3]."""
    h, s, v = rgb2hsv8(rgb)
    s2 = np.minimum(np.maximum(s.astype(F) * F(sf), F(0)), F(255)).astype(np.uint8)        # astype truncates
    return hsv2rgb8(h, s2, v)


def patch_mean(x, bf):
    """x: fp32 [3, P, P] holding u / 255 -> the fp32 mean of x * bf by exact summation of the bytes."""
    u = np.rint(x.astype(F) * F(255)).astype(np.int64)
    return F(np.float64(F(bf)) * (np.float64(int(u.sum())) / (255.0 * u.size)))


def jitter_patch(x, bf, cf, sf):
    """One patch, fp32 [3, P, P] = u / 255 -> fp32 [3, P, P]."""
    x = np.asarray(x, dtype=F)
    bf, cf, sf = F(bf), F(cf), F(sf)
    mean = patch_mean(x, bf)
    x1 = x * bf
    x2 = (x1 - mean) * cf + mean
    c = np.minimum(np.maximum(x2, F(0)), F(1))
    if sf == F(1):
        return c
    q = (c * F(255)).astype(np.uint8)                                   # trunc
    out = saturate8(np.moveaxis(q, 0, -1), sf)
    return np.moveaxis(out, -1, 0).astype(F) / F(255)


def jitter_pairs(lr, hr, table):
    """lr [B,3,p,p], hr [B,3,4p,4p] fp32, table [B,4] = {apply, bf, cf, sf} -> new (lr, hr); apply == 0 rows are copies."""
    lr, hr = np.array(lr, dtype=F, copy=True), np.array(hr, dtype=F, copy=True)
    for b, (ap, bf, cf, sf) in enumerate(np.asarray(table, dtype=F)):
        if ap != 0:
            lr[b] = jitter_patch(lr[b], bf, cf, sf)
            hr[b] = jitter_patch(hr[b], bf, cf, sf)
    return lr, hr
