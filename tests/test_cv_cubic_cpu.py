"""OpenCV's INTER_CUBIC restated (tests/golden/cv_cubic_ref.py, ops.cv_cubic_tables) and the reference's validation size rule
(epoch.val_resized_shape), on the CPU: exact weights, replicated borders, the fp32 form against its fp64 twin, the size rule's cases."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import cv_cubic_ref as R  # noqa: E402

F = np.float32
# (Hi, Wi, Ho, Wo): the GPU test's shapes and the two resizes of the validation fixture
SHAPES = [(1, 1, 3, 2), (2, 3, 5, 7), (9, 7, 2, 3), (40, 24, 16, 9), (160, 96, 64, 36), (33, 21, 33, 21), (5, 8, 20, 32), (5, 8, 20, 31)]
RATIOS = [(1, 1), (1, 3), (2, 5), (3, 7), (7, 3), (9, 2), (24, 9), (40, 16), (8, 32), (8, 31), (21, 21), (510, 128), (339, 85), (2040, 512)]


def test_ops_tables_are_the_restatement():
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    for n_in, n_out in RATIOS:
        idx, wt = ops.cv_cubic_tables(n_in, n_out)
        ridx, rwt = R.tables(n_in, n_out)
        assert idx.dtype == np.int32 and wt.dtype == F and idx.shape == wt.shape == (n_out, 4)
        assert idx.flags.c_contiguous and wt.flags.c_contiguous
        assert np.array_equal(idx, ridx) and wt.tobytes() == rwt.tobytes(), (n_in, n_out)
    for bad in ((0, 4), (4, 0), (-1, 2)):
        with pytest.raises(FFError):
            ops.cv_cubic_tables(*bad)


def test_exact_weights():
    w0 = R._weights(np.array([0.0], dtype=F), F)[0]
    assert w0.tolist() == [0.0, 1.0, 0.0, 0.0]
    wh = R._weights(np.array([0.5], dtype=F), F)[0]
    assert wh.tolist() == [-0.09375, 0.59375, 0.59375, -0.09375]
    for n in (1, 2, 3, 21, 128):                                        # n_in == n_out: x == 0 everywhere, the identity bit for bit
        idx, wt = R.tables(n, n)
        assert np.array_equal(wt, np.tile(np.array([0, 1, 0, 0], dtype=F), (n, 1)))
        assert np.array_equal(idx[:, 1], np.arange(n))
    rng = np.random.default_rng(3)
    img = (rng.standard_normal((2, 33, 21)) * 7).astype(F)              # outside [0, 1]: nothing is clamped
    assert R.resize32(img, 33, 21).tobytes() == img.tobytes()
    # every row sums to 1 within one fp32 rounding (c3 = 1 - c0 - c1 - c2 is itself rounded three times; the row sum is taken in double)
    for n_in, n_out in RATIOS:
        _, wt = R.tables(n_in, n_out)
        assert np.abs(wt.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -23, (n_in, n_out)
        x = R._positions(n_in, n_out)[1]
        assert x.min() >= 0 and x.max() < 1
        assert np.abs(wt).sum(axis=1).max() <= 1.375 + 1e-6             # |c0| + .. + |c3| peaks at x = 0.5


def test_border_taps_replicate():
    for n_in in (1, 2, 3):
        for n_out in (1, 2, 3, 4, 7):
            idx, wt = R.tables(n_in, n_out)
            s = R._positions(n_in, n_out)[0]
            assert idx.min() >= 0 and idx.max() <= n_in - 1
            assert np.array_equal(idx, np.clip(s[:, None] + np.arange(-1, 3), 0, n_in - 1))
            # a constant stays that constant to rounding, whatever the border does
            const = R.resize32(np.full((n_in, n_in), 0.625, dtype=F), n_out, n_out)
            assert np.abs(const - F(0.625)).max() <= 4 * 2.0 ** -24
            # a ramp, by hand: out[d] = sum_k wt[d, k] * ramp[clip(s - 1 + k)], in the restatement's order
            ramp = np.arange(n_in, dtype=F)[None, :] * F(0.25)
            got = R.resize32(ramp, 1, n_out)[0]
            for d in range(n_out):
                v = [ramp[0, min(max(int(s[d]) - 1 + k, 0), n_in - 1)] for k in range(4)]
                want = F(F(F(F(v[0] * wt[d, 0]) + F(v[1] * wt[d, 1])) + F(v[2] * wt[d, 2])) + F(v[3] * wt[d, 3]))
                assert got[d] == want, (n_in, n_out, d)
            # an impulse in the last column: output d is the sum of the weights of the taps that landed on it (clamped ones included)
            imp = np.zeros((1, n_in), dtype=F)
            imp[0, n_in - 1] = 1
            got = R.resize64(imp, 1, n_out)[0]
            _, wt64 = R.tables(n_in, n_out, np.float64)
            for d in range(n_out):
                assert abs(got[d] - wt64[d][idx[d] == n_in - 1].sum()) < 1e-15
    up = R.tables(2, 8)[0]                                              # x4 of two pixels: both borders clamp two taps
    assert up[0].tolist() == [0, 0, 0, 1] and up[-1].tolist() == [0, 1, 1, 1]


def _inputs(Hi, Wi, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (3, Hi, Wi), dtype=np.uint8).astype(F) / F(255), rng.random((3, Hi, Wi), dtype=F)


def test_fp32_restatement_against_fp64():
    """Largest |resize32 - resize64| over these inputs (bytes / 255 and uniform fp32 in [0, 1), every shape of SHAPES), measured on the
    CPU: 8.63e-7 (the fp32 weights carry most of it: c3 = 1 - c0 - c1 - c2 alone is three roundings of values near 1).  The bar is
    four times that; beyond 1e-5 the restatement would be wrong (sixteen products whose absolute weights sum to at most
    1.375^2 ~ 1.9 per output, each rounded at 2^-24 relative)."""
    worst = 0.0
    for i, (Hi, Wi, Ho, Wo) in enumerate(SHAPES):
        for img in _inputs(Hi, Wi, 40 + i):
            a, b = R.resize32(img, Ho, Wo), R.resize64(img, Ho, Wo)
            assert a.dtype == F and b.dtype == np.float64 and a.shape == b.shape == (3, Ho, Wo)
            worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()))
    print("max |fp32 - fp64| =", worst)
    assert worst < 1e-5
    assert worst < 4 * 8.63e-7


def test_resize_is_separable_and_overshoots():
    """Against a plain double loop over taps (no vectorisation to get wrong), and: a step edge overshoots [0, 1] -- values are not clamped."""
    rng = np.random.default_rng(9)
    img = rng.random((9, 7))
    Ho, Wo = 4, 5
    (ih, wh), (iw, ww) = R.tables(9, Ho, np.float64), R.tables(7, Wo, np.float64)
    want = np.zeros((Ho, Wo))
    for y in range(Ho):
        for x in range(Wo):
            want[y, x] = sum(wh[y, j] * ww[x, k] * img[ih[y, j], iw[x, k]] for j in range(4) for k in range(4))
    assert np.abs(R.resize64(img, Ho, Wo) - want).max() < 1e-14
    step = np.zeros((1, 8), dtype=F)
    step[0, 4:] = 1
    out = R.resize32(step, 1, 32)
    assert out.min() < -0.05 and out.max() > 1.05


def test_val_resized_shape():
    from isr2_amd.epoch import val_resized_shape as V
    assert V(510, 339) == (128, 85)                                     # portrait: int(339 * 128 / 510) = int(85.08)
    assert V(339, 510) == (85, 128)
    assert V(200, 200) == (128, 128)                                    # square: the second branch
    assert V(128, 100) is None and V(100, 128) is None and V(1, 1) is None
    assert V(129, 100) == (128, 99)                                     # int(99.22)
    assert V(100, 129) == (99, 128)
    assert V(300, 299) == (128, 127)                                    # 299 * 128 / 300 = 127.57: truncation, rounding would give 128
    assert V(299, 300) == (127, 128)
    assert V(4000, 3000, max_size=None) is None
    assert V(40, 24, max_size=64) == (16, 9) and V(12, 20, max_size=64) == (9, 16) and V(12, 16, max_size=64) is None
    assert V(100, 30, max_size=64, scale=2) == (32, 9)
    # the same rule as the restatement's val_pair
    rng = np.random.default_rng(1)
    for h, w in ((40, 24), (12, 20), (12, 16), (17, 17), (16, 9)):
        lr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        hr = rng.integers(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8)
        a, b = R.val_pair(lr, hr, max_size=64)
        nh, nw = V(h, w, max_size=64) or (h, w)
        assert a.shape == (3, nh, nw) and b.shape == (3, 4 * nh, 4 * nw)
        assert a.min() >= 0 and a.max() <= 1 and b.min() >= 0 and b.max() <= 1
