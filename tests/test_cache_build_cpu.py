"""Host side of the cached-expert data-set builder (isr2_amd.cache.build_from_folders): the crop plan, the weight tables of the
antialiased x1/4 resize against torch on the CPU, and the argument checks of the two new C entry points.  No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F


def test_crop_plan_is_deterministic_inside_and_distinct():
    from isr2_amd.cache import crop_plan
    p = 16
    assert crop_plan(16, 16, p, 1, 0, 0) == [(0, 0)]
    assert set(crop_plan(16, 16, p, 3, 5, 2)) == {(0, 0)}                      # the only position there is
    for h, w in ((16, 16), (17, 40), (23, 37)):
        for seed, index in ((0, 0), (0, 1), (7, 3), (123456789, 4000)):
            for crops in (1, 2, 5):
                plan = crop_plan(h, w, p, crops, seed, index)
                assert plan == crop_plan(h, w, p, crops, seed, index)            # same arguments, same list
                assert len(plan) == crops and all(isinstance(t, int) and isinstance(l, int) for t, l in plan)
                assert all(0 <= t <= h - p and 0 <= l <= w - p for t, l in plan), (h, w, plan)
                if (h - p + 1) * (w - p + 1) >= crops:
                    assert len(set(plan)) == crops, (h, w, seed, index, plan)    # distinct when the image allows
    # every position of a small image is reachable, both ends of both ranges included
    seen = {pos for i in range(400) for pos in crop_plan(17, 19, p, 2, 1, i)}
    assert seen == {(t, l) for t in range(2) for l in range(4)}


def test_crop_plan_center_small_images_and_seeding():
    from isr2_amd.cache import crop_plan
    assert crop_plan(23, 37, 16, 5, 0, 0, center=True) == [(3, 10)]
    assert crop_plan(40, 17, 16, 5, 9, 9, center=True) == [(12, 0)]
    assert crop_plan(16, 16, 16, 2, 0, 0, center=True) == [(0, 0)]
    for h, w in ((15, 40), (40, 15), (12, 12)):
        assert crop_plan(h, w, 16, 2, 0, 0) == [] and crop_plan(h, w, 16, 2, 0, 0, center=True) == []
    base = crop_plan(200, 300, 16, 5, 0, 0)
    assert crop_plan(200, 300, 16, 5, 1, 0) != base                             # another seed
    assert crop_plan(200, 300, 16, 5, 0, 1) != base                             # another image of the same seed
    assert crop_plan(200, 300, 16, 5, 1, 0) != crop_plan(200, 300, 16, 5, 0, 1)
    # no global state: the plan does not depend on, and does not disturb, the module-level generators
    import random
    random.seed(3)
    torch.manual_seed(3)
    a, r1, t1 = crop_plan(200, 300, 16, 5, 0, 0), random.random(), torch.rand(1).item()
    random.seed(3)
    torch.manual_seed(3)
    assert a == base and r1 == random.random() and t1 == torch.rand(1).item()


def _apply_tables(img: np.ndarray, span, wt) -> np.ndarray:
    """One axis (the last) of resize_aa in numpy float32: acc += w_j * x[first + j] in ascending j."""
    out = np.zeros(img.shape[:-1] + (span.shape[0],), dtype=np.float32)
    for i, (lo, n) in enumerate(span):
        acc = np.zeros(img.shape[:-1], dtype=np.float32)
        for j in range(n):
            acc = (acc + wt[i, j] * img[..., lo + j]).astype(np.float32)
        out[..., i] = acc
    return out


@pytest.mark.parametrize("H,W", [(36, 52), (64, 64)])
def test_aa_tables_match_torch_antialiased_bicubic(H, W):
    from isr2_amd.ops import aa_tables, AA_TAPS
    img = np.random.default_rng(H * 1000 + W).integers(0, 256, (3, H, W)).astype(np.float32) / np.float32(255.0)
    tabs = {}
    for n in {H, W}:
        span, wt = aa_tables(n, n // 4)
        assert span.dtype == np.int32 and wt.dtype == np.float32 and span.shape == (n // 4, 2) and wt.shape == (n // 4, AA_TAPS)
        assert AA_TAPS == 16 and span[:, 1].max() <= 16 and span[:, 1].min() >= 1     # no row has more than 16 taps
        assert (span[:, 0] >= 0).all() and (span[:, 0] + span[:, 1] <= n).all()
        assert np.abs(wt.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6           # every row sums to 1
        assert all((wt[i, span[i, 1]:] == 0).all() for i in range(n // 4))             # zero padded
        assert np.abs(wt).astype(np.float64).sum(axis=1).max() <= 1.172 + 1e-3         # the bound the fp32 tolerance is built on
        tabs[n] = (span, wt)
    hor = _apply_tables(img, *tabs[W])                                                 # horizontal pass first
    got = _apply_tables(hor.transpose(0, 2, 1), *tabs[H]).transpose(0, 2, 1)
    ref = F.interpolate(torch.from_numpy(img)[None], size=(H // 4, W // 4), mode="bicubic", antialias=True, align_corners=False)[0].numpy()
    err = float(np.abs(got - ref).max())
    print(f"aa tables {H}x{W}: max |numpy - torch| = {err:.3e}")
    assert err <= 6e-6


def test_aa_tables_refuse_what_the_kernel_cannot_hold():
    from isr2_amd.lib import FFError
    from isr2_amd.ops import aa_tables
    with pytest.raises(FFError):
        aa_tables(64, 8)                                                               # x1/8: 32 taps
    with pytest.raises(FFError):
        aa_tables(8, 16)
    with pytest.raises(FFError):
        aa_tables(8, 0)


def test_new_entry_points_validate_arguments_without_a_gpu():
    from isr2_amd import lib as L
    lib = L.load()
    assert lib.ff_abi_version() == 7
    # ff_crop_pairs_u8(lr_u8, hr_u8, h, w, pos, K, p, lr_out, hr_out, stream): null pointers, then bad sizes (1 = a non-null dummy
    # address: every check happens before anything is dereferenced or launched)
    for args in ((None, 1, 23, 37, 1, 3, 8, 1, 1), (1, None, 23, 37, 1, 3, 8, 1, 1), (1, 1, 23, 37, None, 3, 8, 1, 1),
                 (1, 1, 23, 37, 1, 3, 8, None, 1), (1, 1, 23, 37, 1, 3, 8, 1, None),
                 (1, 1, 23, 37, 1, 0, 8, 1, 1), (1, 1, 23, 37, 1, 3, 0, 1, 1), (1, 1, 23, 37, 1, 3, 24, 1, 1), (1, 1, 0, 37, 1, 3, 8, 1, 1)):
        assert lib.ff_crop_pairs_u8(*args, None) != 0 and b"ff_crop_pairs_u8" in lib.ff_last_error(), args
    # ff_resize_aa(in, out, planes, Hi, Wi, Ho, Wo, span_w, wt_w, span_h, wt_h, stream)
    for args in ((None, 1, 3, 64, 64, 16, 16, 16, 16, 16, 16), (16, None, 3, 64, 64, 16, 16, 16, 16, 16, 16),
                 (16, 16, 3, 64, 64, 16, 16, None, 16, 16, 16), (16, 16, 3, 64, 64, 16, 16, 16, 16, 16, None),
                 (16, 16, 0, 64, 64, 16, 16, 16, 16, 16, 16), (16, 16, 3, 64, 64, 0, 16, 16, 16, 16, 16),
                 (16, 16, 3, 64, 64, 32, 32, 16, 16, 16, 16), (16, 16, 3, 65, 64, 16, 16, 16, 16, 16, 16),
                 (16, 16, 3, 64, 60, 16, 16, 16, 16, 16, 16)):
        assert lib.ff_resize_aa(*args, None) != 0 and b"ff_resize_aa" in lib.ff_last_error(), args


def test_wrappers_refuse_cpu_tensors():
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    with pytest.raises(FFError):
        ops.crop_pairs_u8(torch.zeros(16, 16, 3, dtype=torch.uint8), torch.zeros(64, 64, 3, dtype=torch.uint8), [(0, 0)], 16)
    with pytest.raises(FFError):
        ops.resize_aa(torch.zeros(1, 3, 64, 64), (16, 16))
