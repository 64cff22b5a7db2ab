"""Host side of the live loop's colour jitter: the numpy restatement (tests/golden/jitter_ref.py) against the vectors of its definition,
epoch.live_jitter_plan, live_plan's unchanged draws, and the argument checks of ff_color_jitter_pairs and its wrapper.  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import jitter_ref as J  # noqa: E402

F = np.float32
# RGB, its HSV (None: not part of the vector), sf, RGB after the whole saturation step
VECTORS = [((200, 100, 50), (10, 191, 200), 1.2, (200, 80, 20)),
           ((200, 100, 50), (10, 191, 200), 0.8, (200, 121, 81)),
           ((10, 200, 250), (96, 245, 250), 1.2, (0, 200, 250)),
           ((37, 91, 12), (50, 221, 91), 1.1, (33, 91, 4)),
           ((255, 0, 0), None, 0.8, (255, 51, 51)),
           ((100, 100, 100), None, 1.2, (100, 100, 100)),
           ((0, 255, 0), None, 1.0, (0, 255, 0))]


@pytest.mark.parametrize("rgb,hsv,sf,want", VECTORS)
def test_the_seven_vectors(rgb, hsv, sf, want):
    q = np.array(rgb, dtype=np.uint8)
    if hsv is not None:
        assert tuple(int(a) for a in J.rgb2hsv8(q)) == hsv
    assert tuple(int(a) for a in J.saturate8(q, sf)) == want


def test_tables_are_the_rounded_quotients():
    assert J.SDIV[0] == 0 and J.HDIV[0] == 0 and J.SDIV[255] == 4096 and J.SDIV[1] == 255 * 4096 and J.HDIV[1] == 122880
    for i in range(1, 256):                                             # exact integer rounding, ties to even
        for tab, n, d in ((J.SDIV, 255 * 4096, i), (J.HDIV, 180 * 4096, 6 * i)):
            q, r = divmod(n, d)
            assert tab[i] == q + (1 if 2 * r > d or (2 * r == d and q & 1) else 0)


def test_grey_pixels_are_fixed_points_for_any_sf():
    g = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    for sf in (0.8, 0.93, 1.0, 1.07, 1.2):
        assert np.array_equal(J.saturate8(g, sf), g), sf


def test_sat_clips_at_255():
    q = np.array([[255, 0, 0], [0, 0, 255], [10, 200, 250], [3, 250, 1]], dtype=np.uint8)
    _, s, _ = J.rgb2hsv8(q)
    assert (s.astype(F) * F(1.2) > 255).all()                           # every one of them would leave the byte
    h, _, v = J.rgb2hsv8(q)
    assert np.array_equal(J.saturate8(q, 1.2), J.hsv2rgb8(h, np.full_like(s, 255), v))
    assert tuple(J.saturate8(q[0], 1.2)) == (255, 0, 0)
    rng = np.random.default_rng(0)
    allq = rng.integers(0, 256, (20000, 3), dtype=np.uint8)
    hh, ss, vv = J.rgb2hsv8(allq)
    assert hh.min() >= 0 and hh.max() <= 179 and ss.min() >= 0 and ss.max() <= 255 and np.array_equal(vv, allq.max(axis=1))
    back = J.hsv2rgb8(hh, ss, vv).astype(np.int64)
    assert np.abs(back - allq).max() <= 5                               # hue is stored in 2-degree steps


def test_sf_one_takes_the_float_path_without_quantisation():
    rng = np.random.default_rng(1)
    x = (rng.integers(0, 256, (3, 5, 5)).astype(F) / F(255))
    bf, cf = F(0.9), F(1.1)
    out = J.jitter_patch(x, bf, cf, 1.0)
    mean = J.patch_mean(x, bf)
    want = np.clip((x * bf - mean) * cf + mean, F(0), F(1))
    assert out.dtype == F and np.array_equal(out, want)
    assert (np.abs(out * F(255) - np.rint(out * F(255))) > 1e-3).any()  # values between the byte levels survive
    q = J.jitter_patch(x, bf, cf, 1.0000001)                            # the next float: the 8-bit path
    assert np.array_equal(q, np.rint(q * F(255)).astype(F) / F(255))
    # the mean is the exact one: float64 sum of the bytes
    u = np.rint(x * F(255)).astype(np.int64)
    assert mean == F(np.float64(bf) * (u.sum() / (255.0 * 75)))


def test_apply_zero_is_the_identity():
    rng = np.random.default_rng(2)
    lr = rng.integers(0, 256, (2, 3, 4, 4)).astype(F) / F(255)
    hr = rng.integers(0, 256, (2, 3, 16, 16)).astype(F) / F(255)
    a, b = J.jitter_pairs(lr, hr, [[0, 0.8, 1.2, 1.2], [1, 0.8, 1.2, 1.2]])
    assert np.array_equal(a[0], lr[0]) and np.array_equal(b[0], hr[0])
    assert not np.array_equal(a[1], lr[1]) and not np.array_equal(b[1], hr[1])
    assert np.array_equal(b[1], J.jitter_patch(hr[1], 0.8, 1.2, 1.2))


def test_live_jitter_plan_is_a_function_of_seed_and_epoch_inside_its_ranges():
    from isr2_amd.epoch import live_jitter_plan
    from isr2_amd.lib import FFError
    a = live_jitter_plan(50, 4, 11, 3)
    assert a.shape == (50, 4, 4) and a.dtype == np.float32
    assert np.array_equal(a, live_jitter_plan(50, 4, 11, 3))
    for other in (live_jitter_plan(50, 4, 11, 4), live_jitter_plan(50, 4, 12, 3)):
        assert not np.array_equal(a[..., 0], other[..., 0]) and not np.array_equal(a[..., 1:], other[..., 1:])
    assert set(np.unique(a[..., 0]).tolist()) == {0.0, 1.0}
    assert 0.35 <= float(a[..., 0].mean()) <= 0.65                      # 200 fair draws: 0.5 +- 4.2 sigma
    lo, hi = F(1.0 - 0.2), F(1.0 + 0.2)
    assert (a[..., 1:] >= lo).all() and (a[..., 1:] <= hi).all()
    assert a[..., 1:].min() < 0.85 and a[..., 1:].max() > 1.15          # the range is used
    assert not np.array_equal(a[..., 1], a[..., 2]) and not np.array_equal(a[..., 2], a[..., 3])
    b = live_jitter_plan(20, 3, 0, 0, prob=1.0, brightness=0.05, contrast=0.0, saturation=0.3)
    assert (b[..., 0] == 1).all() and (b[..., 2] == 1).all()
    assert (np.abs(b[..., 1] - 1) <= F(0.05) + 1e-7).all() and (b[..., 3] >= F(0.7)).all() and (b[..., 3] <= F(1.3)).all()
    assert (live_jitter_plan(20, 3, 0, 0, prob=0.0)[..., 0] == 0).all()
    # the documented draws: live_plan's key, counters 6..9
    key = [11, 3]
    gen = lambda c: np.random.Generator(np.random.Philox(key=key, counter=[0, 0, 0, c]))     # noqa: E731
    assert np.array_equal(a[..., 0].reshape(-1), (gen(6).random(200) < 0.5).astype(F))
    for j in range(3):
        assert np.array_equal(a[..., 1 + j].reshape(-1), (1.0 + gen(7 + j).uniform(-0.2, 0.2, size=200)).astype(F))
    state = np.random.get_state()[1].copy()                             # no global generator is touched
    live_jitter_plan(5, 2, 1, 1)
    assert np.array_equal(state, np.random.get_state()[1])
    for bad in (dict(prob=1.5), dict(brightness=1.0), dict(saturation=-0.1)):
        with pytest.raises(FFError):
            live_jitter_plan(5, 2, 0, 0, **bad)
    with pytest.raises(FFError):
        live_jitter_plan(5, 0, 0, 0)


def test_live_plan_still_returns_its_documented_draws():
    """live_plan's streams are counters 0..5 of the (seed, epoch) key; the jitter table's 6..9 leave them as they were."""
    from isr2_amd.epoch import live_plan
    sizes = [(16, 16), (24, 40), (33, 28), (16, 70), (61, 17)]
    R, B, p, seed, epoch = 7, 4, 16, 3, 2
    idx, top, left, codes = live_plan(sizes, R, B, p, seed, epoch)
    gen = lambda c: np.random.Generator(np.random.Philox(key=[seed, epoch], counter=[0, 0, 0, c]))     # noqa: E731
    n = len(sizes) * R
    m = n // B * B
    order = gen(0).permutation(n)[:m].astype(np.int64)
    room = np.asarray(sizes, dtype=np.int64)[order % len(sizes)] - p
    w_top = gen(1).integers(0, room[:, 0] + 1, dtype=np.int64)
    w_left = gen(2).integers(0, room[:, 1] + 1, dtype=np.int64)
    flips = gen(3).integers(0, 4, size=m, dtype=np.int64)
    turn = gen(4).integers(0, 2, size=m, dtype=np.int64)
    k = np.where(turn == 1, gen(5).integers(1, 4, size=m, dtype=np.int64), 0)
    shp = (n // B, B)
    assert np.array_equal(idx, order.reshape(shp)) and np.array_equal(top, w_top.reshape(shp)) and np.array_equal(left, w_left.reshape(shp))
    assert np.array_equal(codes, (flips | (k << 2)).astype(np.int32).reshape(shp)) and codes.dtype == np.int32


def test_color_jitter_entry_refuses_nulls_bad_sizes_and_a_short_workspace_without_a_gpu():
    from isr2_amd import lib as L
    lib = L.load()
    assert lib.ff_abi_version() == 7
    assert lib.ff_color_jitter_workspace(0) == -1 and lib.ff_color_jitter_workspace(-3) == -1
    need = lib.ff_color_jitter_workspace(2)
    assert need > 0 and need % 8 == 0 and lib.ff_color_jitter_workspace(14) == 7 * need
    # ff_color_jitter_pairs(lr, hr, table, B, p, workspace, workspace_bytes, stream); 16 = a non-null dummy address, nothing is
    # dereferenced or launched
    for args in ((None, 16, 16, 2, 8, 16, need), (16, None, 16, 2, 8, 16, need), (16, 16, None, 2, 8, 16, need), (16, 16, 16, 2, 8, None, need),
                 (16, 16, 16, 0, 8, 16, need), (16, 16, 16, -1, 8, 16, need), (16, 16, 16, 2, 0, 16, need), (16, 16, 16, 2, 8, 16, need - 1),
                 (16, 16, 16, 2, 8, 16, 0), (16, 16, 16, 2, 8200, 16, need), (16, 16, 16, (1 << 20) + 1, 8, 16, 1 << 40)):
        assert lib.ff_color_jitter_pairs(*args, None) != 0 and b"ff_color_jitter_pairs" in lib.ff_last_error(), args


def test_color_jitter_wrapper_refuses_cpu_tensors():
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    with pytest.raises(FFError):
        ops.color_jitter_pairs(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 16, 16), [[1, 1.0, 1.0, 1.0]])
