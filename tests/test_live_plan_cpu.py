"""Host side of live-expert training (isr2_amd.epoch: live_plan, pool_layout / pool_members) and the argument checks of the sampler's C
entry point and wrapper.  No GPU needed."""
import numpy as np
import pytest
import torch

SIZES = [(16, 16), (24, 40), (33, 28), (16, 70), (61, 17)]              # LR (h, w); the first one IS the patch


def test_live_plan_shapes_ranges_and_image_of_an_entry():
    from isr2_amd.epoch import live_plan
    p, B, R = 16, 4, 7
    idx, top, left, codes = live_plan(SIZES, R, B, p, seed=3, epoch=0)
    nb = len(SIZES) * R // B
    assert nb == 8 and len(SIZES) * R % B == 3                          # 35 entries: the last three are dropped
    for a in (idx, top, left, codes):
        assert a.shape == (nb, B)
    flat = idx.reshape(-1)
    assert len(set(flat.tolist())) == nb * B and flat.min() >= 0 and flat.max() < len(SIZES) * R
    assert sorted(flat.tolist()) != flat.tolist()                       # shuffled
    hw = np.array(SIZES)[idx % len(SIZES)]                              # entry i reads image i % n
    assert (top >= 0).all() and (left >= 0).all() and (top <= hw[..., 0] - p).all() and (left <= hw[..., 1] - p).all()
    assert (top[hw[..., 0] == p] == 0).all() and (left[hw[..., 1] == p] == 0).all()      # h == p: the only position
    assert (codes >= 0).all() and (codes < 16).all()
    # both ends of both ranges are reached, and every image is visited `repeat` times up to the dropped tail
    seen_t, seen_l = set(), set()
    for e in range(40):
        i, t, l, _ = live_plan(SIZES, R, B, p, 3, e)
        m = (i % len(SIZES)) == 1                                       # the 24 x 40 image: top in 0..8, left in 0..24
        seen_t |= set(t[m].tolist())
        seen_l |= set(l[m].tolist())
    assert seen_t == set(range(9)) and seen_l == set(range(25))
    idx_ns, *_ = live_plan(SIZES, R, B, p, 3, 0, shuffle=False)
    assert idx_ns.reshape(-1).tolist() == list(range(nb * B))


def test_live_plan_is_a_function_of_seed_and_epoch():
    from isr2_amd.epoch import live_plan
    a = live_plan(SIZES, 6, 2, 16, 11, 4)
    b = live_plan(SIZES, 6, 2, 16, 11, 4)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = live_plan(SIZES, 6, 2, 16, 11, 5)
    d = live_plan(SIZES, 6, 2, 16, 12, 4)
    for other in (c, d):
        assert not np.array_equal(a[0], other[0]) and not np.array_equal(a[3], other[3])
        assert not (np.array_equal(a[1], other[1]) and np.array_equal(a[2], other[2]))
    state = np.random.get_state()[1].copy()                             # no global generator is touched
    live_plan(SIZES, 6, 2, 16, 11, 4)
    assert np.array_equal(state, np.random.get_state()[1])


def test_live_plan_without_augmentation_is_the_centre_crop():
    from isr2_amd.epoch import live_plan
    idx, top, left, codes = live_plan(SIZES, 3, 2, 16, 0, 0, augment=False)
    assert (codes == 0).all()
    hw = np.array(SIZES)[idx % len(SIZES)]
    assert np.array_equal(top, (hw[..., 0] - 16) // 2) and np.array_equal(left, (hw[..., 1] - 16) // 2)
    assert live_plan([(23, 37)], 1, 1, 16, 0, 0, augment=False)[1:3] == (np.array([[3]]), np.array([[10]]))


def test_live_plan_rotation_is_the_references_half_and_thirds():
    """k = 0 with p = 0.5, else uniform in {1, 2, 3}: over 60 000 draws of seed 0 the share of k = 0 lies in [0.49, 0.51] (sigma =
    0.00204) and every other k in [0.155, 0.178] (1/6 +- 0.0115, sigma = 0.00152): about +-5 sigma, and deterministic for the seed.
    The flips are fair and independent of k."""
    from isr2_amd.epoch import live_plan
    _, _, _, codes = live_plan([(16, 16)] * 10, 6000, 60, 16, seed=0, epoch=0)
    c = codes.reshape(-1)
    assert c.size == 60000
    k = c >> 2
    share = [float((k == v).mean()) for v in range(4)]
    print("k shares", share, "hflip", float((c & 1).mean()), "vflip", float(((c >> 1) & 1).mean()))
    assert 0.49 <= share[0] <= 0.51
    assert all(0.155 <= s <= 0.178 for s in share[1:])
    assert 0.49 <= float((c & 1).mean()) <= 0.51 and 0.49 <= float(((c >> 1) & 1).mean()) <= 0.51
    assert 0.24 <= float(((c & 3) == 3).mean()) <= 0.26                  # both flips: a quarter


def test_live_plan_refuses_bad_arguments():
    from isr2_amd.epoch import live_plan
    from isr2_amd.lib import FFError
    for args in (([], 1, 1, 16), (SIZES, 0, 1, 16), (SIZES, 1, 0, 16), (SIZES, 1, 1, 0), (SIZES + [(15, 40)], 1, 1, 16)):
        with pytest.raises(FFError):
            live_plan(*args, 0, 0)


def test_pool_layout_is_packed_and_small_images_are_left_out():
    from isr2_amd.epoch import pool_layout, pool_members
    from isr2_amd.lib import FFError
    sizes = [(37, 53), (12, 40), (64, 64), (70, 41), (40, 15)]
    keep, skipped = pool_members(sizes, 16)
    assert keep == [0, 2, 3] and skipped == 2                           # smaller than the patch in either axis: absent, counted
    assert pool_members(sizes, 37) == ([0, 2, 3], 2) and pool_members(sizes, 38) == ([2, 3], 3)
    kept = [sizes[i] for i in keep]
    offs, total = pool_layout(kept)
    assert offs.dtype == np.int64 and offs.shape == (3, 2)
    n = 0
    for (h, w), (lo, ho) in zip(kept, offs.tolist()):
        assert lo == n and ho == n + 3 * h * w                          # LR then HR, back to back, no padding
        n = ho + 3 * (4 * h) * (4 * w)
    assert total == n == 51 * (37 * 53 + 64 * 64 + 70 * 41)
    assert offs[1, 0] % 2 == 1 and offs[1, 1] % 2 == 1                  # nothing is aligned
    assert pool_layout([])[1] == 0
    big = pool_layout([(1356, 2040)] * 900)[1]                          # DF2K-sized: past 2^31, still exact
    assert big == 900 * 51 * 1356 * 2040 and big > 2 ** 31
    with pytest.raises(FFError):
        pool_layout([(0, 5)])
    with pytest.raises(FFError):
        pool_members(sizes, 0)


def test_sample_pairs_entry_refuses_nulls_and_empty_sizes_without_a_gpu():
    from isr2_amd import lib as L
    lib = L.load()
    assert lib.ff_abi_version() == 7
    # ff_sample_pairs_u8(pool, desc, B, p, lr_out, hr_out, stream); 16 = a non-null dummy address, nothing is dereferenced or launched
    for args in ((None, 16, 2, 8, 16, 16), (16, None, 2, 8, 16, 16), (16, 16, 2, 8, None, 16), (16, 16, 2, 8, 16, None),
                 (16, 16, 0, 8, 16, 16), (16, 16, 2, 0, 16, 16), (16, 16, -1, 8, 16, 16)):
        assert lib.ff_sample_pairs_u8(*args, None) != 0 and b"ff_sample_pairs_u8" in lib.ff_last_error(), args


def test_sample_pairs_wrapper_refuses_cpu_tensors():
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    with pytest.raises(FFError):
        ops.sample_pairs_u8(torch.zeros(51 * 16 * 16, dtype=torch.uint8), [[0, 768, 16, 16, 0, 0, 0, 0]], 16)
