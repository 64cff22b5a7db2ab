"""numpy restatement of the resize that csrc/resample.hip's resize_cv_cubic_kernel applies (ops.resize_cv_cubic), the reference's
cv2.resize(img, (w, h), interpolation=cv2.INTER_CUBIC) in ValidationDataset (dataset.py:473-506) restated from OpenCV's published
definition (imgproc/resize.cpp: the per-axis table of cv::resize for INTER_CUBIC, and interpolateCubic):

    scale = double(n_in) / n_out;  f = float((d + 0.5) * scale - 0.5) (double arithmetic, one rounding to fp32);  s = floor(f);  x = f - s
    taps s - 1 .. s + 2, each clamped to [0, n_in - 1] (BORDER_REPLICATE); four taps whatever the ratio: no antialiasing
    A = -0.75f;  c0 = ((A (x + 1) - 5 A)(x + 1) + 8 A)(x + 1) - 4 A;  c1 = ((A + 2) x - (A + 3)) x x + 1;
    c2 = ((A + 2)(1 - x) - (A + 3))(1 - x)(1 - x) + 1;  c3 = 1 - c0 - c1 - c2                                  -- all fp32
    per source row  h = ((v0 a0 + v1 a1) + v2 a2) + v3 a3   (horizontal weights a),  then
    out = ((h0 b0 + h1 b1) + h2 b2) + h3 b3                 (vertical weights b);  no clamping of values

Every fp32 step is one numpy operation on float32 arrays (no fused multiply-add).  OpenCV builds differ in whether their row and column
filters fuse the multiply-adds, and OpenCV is not a dependency here: whether this equals an OpenCV binary to the last bit is pinned
nowhere -- parity unpinned (OpenCV absent).  resize64 is the same function with the weights and the sums in double, the yardstick of
the fp32 form's rounding."""
import numpy as np

F = np.float32


def _positions(n_in, n_out):
    scale = float(n_in) / float(n_out)
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f)
    return s.astype(np.int64), (f - s).astype(F)


def _weights(x, dt):
    x = x.astype(dt)
    A, one = dt(-0.75), dt(1)
    x1, u = x + one, one - x
    c0 = ((A * x1 - dt(5) * A) * x1 + dt(8) * A) * x1 - dt(4) * A
    c1 = ((A + dt(2)) * x - (A + dt(3))) * x * x + one
    c2 = ((A + dt(2)) * u - (A + dt(3))) * u * u + one
    c3 = one - c0 - c1 - c2
    return np.stack([c0, c1, c2, c3], axis=1).astype(dt)


def tables(n_in, n_out, dt=F):
    """-> (idx int32 [n_out, 4], wt dt [n_out, 4]) of one axis.  The position f is fp32 in both forms (it is OpenCV's definition, not
    rounding noise); dt is the precision of the weights."""
    s, x = _positions(n_in, n_out)
    idx = np.clip(s[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1).astype(np.int32)
    return idx, _weights(x, dt)


def _resize(img, Ho, Wo, dt):
    img = np.asarray(img).astype(dt)
    Hi, Wi = img.shape[-2:]
    iw, ww = tables(Wi, Wo, dt)
    ih, wh = tables(Hi, Ho, dt)
    v = img[..., :, iw]                                                 # [..., Hi, Wo, 4]
    h = ((v[..., 0] * ww[:, 0] + v[..., 1] * ww[:, 1]) + v[..., 2] * ww[:, 2]) + v[..., 3] * ww[:, 3]          # [..., Hi, Wo]
    r = np.moveaxis(h[..., ih, :], -2, -1)                              # [..., Ho, Wo, 4]
    out = ((r[..., 0] * wh[:, 0, None] + r[..., 1] * wh[:, 1, None]) + r[..., 2] * wh[:, 2, None]) + r[..., 3] * wh[:, 3, None]
    assert out.dtype == dt and out.shape[-2:] == (Ho, Wo)
    return out


def resize32(img, Ho, Wo):
    """[..., Hi, Wi] -> float32 [..., Ho, Wo], the kernel's arithmetic in its order."""
    return _resize(img, Ho, Wo, F)


def resize64(img, Ho, Wo):
    """The same taps and positions, weights and sums in float64."""
    return _resize(img, Ho, Wo, np.float64)


def val_pair(lr_u8, hr_u8, max_size=512, scale=4):
    """ValidationDataset.__getitem__ (dataset.py:473-506) on one uint8 HWC pair -> (lr, hr) float32 CHW in [0, 1]: u8 / 255, the resize
    when the LR's longer side exceeds max_size // scale (Python float division, then truncation; a square image takes the second
    branch), clip(0, 1)."""
    lr = np.moveaxis(lr_u8.astype(F) / F(255), -1, 0)
    hr = np.moveaxis(hr_u8.astype(F) / F(255), -1, 0)
    h, w = lr.shape[-2:]
    if max_size is not None and max(h, w) > max_size // scale:
        if h > w:
            nh = max_size // scale
            nw = int(w * nh / h)
        else:
            nw = max_size // scale
            nh = int(h * nw / w)
        lr, hr = resize32(lr, nh, nw), resize32(hr, nh * scale, nw * scale)
    return np.ascontiguousarray(np.clip(lr, F(0), F(1))), np.ascontiguousarray(np.clip(hr, F(0), F(1)))
