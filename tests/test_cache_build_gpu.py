"""Device side of the cached-expert data-set builder: ff_crop_pairs_u8 and ff_resize_aa against torch, and
cache.build_from_folders end to end against the sequential cache.extract loop (bit for bit)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _u8(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def model(synth_sd):
    _need_gpu()
    from isr2_amd import ops
    from isr2_amd.model import FreqFusionHIP
    ops.set_gemm_mode("bf16x3")
    return FreqFusionHIP(synth_sd, "cuda:0")


# ---- crop_pairs_u8 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,p,positions", [(23, 37, 8, [(0, 0), (15, 29), (7, 13)]),      # w % 4 != 0; far corner; odd offsets
                                             (16, 16, 16, [(0, 0)]),                            # the patch is the image
                                             (23, 37, 7, [(16, 30), (1, 2)])])                  # p % 4 != 0: the scalar-store LR path
def test_crop_pairs_u8_equals_slicing(h, w, p, positions):
    _need_gpu()
    from isr2_amd import ops
    lr_u8, hr_u8 = torch.from_numpy(_u8(1, h, w)).cuda(), torch.from_numpy(_u8(2, 4 * h, 4 * w)).cuda()
    lr_full, hr_full = ops.u8_to_f32_image(lr_u8), ops.u8_to_f32_image(hr_u8)
    lr, hr = ops.crop_pairs_u8(lr_u8, hr_u8, positions, p)
    assert tuple(lr.shape) == (len(positions), 3, p, p) and tuple(hr.shape) == (len(positions), 3, 4 * p, 4 * p)
    for k, (t, l) in enumerate(positions):
        assert torch.equal(lr[k], lr_full[0, :, t:t + p, l:l + p]), (k, t, l)
        assert torch.equal(hr[k], hr_full[0, :, 4 * t:4 * (t + p), 4 * l:4 * (l + p)]), (k, t, l)
    assert torch.equal(lr_full.cpu()[0], torch.from_numpy(_u8(1, h, w)).permute(2, 0, 1).float() / 255.0)


def test_crop_pairs_u8_refuses_before_any_launch(monkeypatch):
    _need_gpu()
    from isr2_amd import lib as L, ops
    lr_u8, hr_u8 = torch.from_numpy(_u8(1, 23, 37)).cuda(), torch.from_numpy(_u8(2, 92, 148)).cuda()
    calls = []
    real = L.load().ff_crop_pairs_u8

    class Spy:                                                      # stands in for the library: counts what reaches the C entry point
        def __getattr__(self, name):
            return getattr(L.load(), name)

        def ff_crop_pairs_u8(self, *a):
            calls.append(a)
            return real(*a)

    monkeypatch.setattr(ops, "_L", lambda: Spy())
    for pos, p in (([(16, 29)], 8), ([(15, 30)], 8), ([(0, 0), (-1, 0)], 8), ([], 8), ([(0, 0)], 24), ([(0, 0)], 0)):
        with pytest.raises(L.FFError):
            ops.crop_pairs_u8(lr_u8, hr_u8, pos, p)
    with pytest.raises(L.FFError):
        ops.crop_pairs_u8(lr_u8, hr_u8[:91].contiguous(), [(0, 0)], 8)        # hr not exactly 4x lr
    with pytest.raises(L.FFError):
        ops.crop_pairs_u8(lr_u8.float(), hr_u8, [(0, 0)], 8)
    assert calls == []
    ops.crop_pairs_u8(lr_u8, hr_u8, [(15, 29)], 8)
    assert len(calls) == 1


# ---- resize_aa -----------------------------------------------------------------------------------------------------------------------
def _hard_edges(H, W):
    """Checkerboard of 3-pixel squares in one plane, a vertical and a diagonal step in the others: overshoot outside [0,1]."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([((y // 3 + x // 3) % 2) * 255, (x >= W // 2 + 1) * 255, (x + y > (H + W) // 2) * 255], axis=-1)
    return img.astype(np.uint8)


@pytest.mark.parametrize("H,W", [(52, 76), (256, 192), (36, 52)])      # smaller than one tile; several tiles both ways; 9 x 13
def test_resize_aa_matches_torch(H, W):
    _need_gpu()
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    imgs = np.stack([_u8(H + W, H, W), _hard_edges(H, W)])                                 # [2,H,W,3]
    x = (torch.from_numpy(imgs).permute(0, 3, 1, 2).float() / 255.0).contiguous()
    ref = F.interpolate(x, size=(H // 4, W // 4), mode="bicubic", antialias=True, align_corners=False)
    assert ref.min().item() < 0.0 and ref.max().item() > 1.0                               # the hard edges do overshoot
    got = ops.resize_aa(x.cuda(), (H // 4, W // 4))
    assert tuple(got.shape) == (2, 3, H // 4, W // 4)
    err = (got.cpu() - ref).abs().max().item()
    q_got = torch.stack([ops.f32_to_u8_image(got[b]).cpu() for b in range(2)]).int()
    q_ref = torch.stack([ops.f32_to_u8_image(ref[b].cuda()).cpu() for b in range(2)]).int()
    lev = (q_got - q_ref).abs()
    print(f"resize_aa {H}x{W}: max |hip - torch| = {err:.3e}, uint8 levels differing {int((lev > 0).sum())} of {lev.numel()}")
    assert err <= 6e-6
    assert lev.max().item() <= 1 and (lev > 0).float().mean().item() <= 1e-3
    with pytest.raises(FFError):
        ops.resize_aa(x.cuda(), (H // 2, W // 2))
    with pytest.raises(FFError):
        ops.resize_aa(x.cuda()[:, :, :H - 1].contiguous(), (H // 4, W // 4))
    with pytest.raises(FFError):
        ops.resize_aa(x.cuda().permute(0, 1, 3, 2), (W // 4, H // 4))                          # not contiguous


# ---- build_from_folders ----------------------------------------------------------------------------------------------------------
def _save(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def _load_parts(d, stem):
    from isr2_amd import cache
    return [torch.load(os.path.join(d, stem + s), weights_only=True) for s in (cache.PRIMARY_SUFFIX, cache.REST_SUFFIX)]


def _assert_same(a, b, where):
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), where
        for k in a:
            _assert_same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    else:
        assert a == b, where


PAIRS = (("a_wide", 23, 37), ("b_one", 16, 16), ("c_tall", 40, 17))


@pytest.fixture(scope="module")
def pair_folders(tmp_path_factory):
    root = tmp_path_factory.mktemp("pairs")
    os.makedirs(root / "lr")
    os.makedirs(root / "hr")
    for i, (stem, h, w) in enumerate(PAIRS + (("d_small", 12, 12),)):
        _save(str(root / "lr" / f"{stem}.png"), _u8(10 + i, h, w))
        _save(str(root / "hr" / f"{stem}.png"), _u8(20 + i, 4 * h, 4 * w))
    return root


@pytest.mark.parametrize("graph", [True, False])              # the three-stream expert pass replayed from one HIP graph / launched
def test_build_from_folders_writes_what_extract_writes(model, pair_folders, tmp_path, graph):
    from isr2_amd import cache, ops
    out, ref = str(tmp_path / "built"), str(tmp_path / "ref")
    res = cache.build_from_folders(model, str(pair_folders / "hr"), out, lr_dir=str(pair_folders / "lr"), patch=16, crops=2, seed=3, graph=graph)
    assert res["graph"] is graph and res["images"] == 3 and res["images_skipped"] == 1 and res["patches_written"] == 6 and res["patches_per_s"] > 0
    assert set(res["seconds"]) >= {"total", "decode", "device", "write"}
    stems = [f"{s}_p{k}" for s, _, _ in PAIRS for k in range(2)]
    assert cache.list_stems(out) == sorted(stems)
    assert sorted(os.listdir(out)) == sorted(s + suf for s in stems for suf in (cache.PRIMARY_SUFFIX, cache.REST_SUFFIX))   # no temporaries left
    # the sequential loop over the same patches, cut with torch slicing at the plan's positions (image index = sorted order)
    samples = []
    for index, (stem, h, w) in enumerate(PAIRS):
        lr = ops.u8_to_f32_image(torch.from_numpy(_u8(10 + index, h, w)).cuda())
        hr = ops.u8_to_f32_image(torch.from_numpy(_u8(20 + index, 4 * h, 4 * w)).cuda())
        plan = cache.crop_plan(h, w, 16, 2, 3, index)
        assert len(plan) == 2
        for k, (t, l) in enumerate(plan):
            samples.append((f"{stem}_p{k}", lr[:, :, t:t + 16, l:l + 16].contiguous(), hr[0, :, 4 * t:4 * t + 64, 4 * l:4 * l + 64].contiguous()))
    assert cache.extract(model, samples, ref) == 6
    for s in stems:
        for got, want in zip(_load_parts(out, s), _load_parts(ref, s)):
            _assert_same(got, want, s)
        smp = cache.read_sample(out, s)
        assert smp["filename"] == s and tuple(smp["lr"].shape) == (3, 16, 16) and tuple(smp["hr"].shape) == (3, 64, 64)
        assert tuple(smp["expert_imgs"]["dat"].shape) == (3, 64, 64) and tuple(smp["expert_feats"]["nafnet"].shape) == (64, 16, 16)


def test_build_from_folders_refuses_a_pair_that_is_not_x4(model, pair_folders, tmp_path):
    import shutil
    hr, lr = tmp_path / "hr", tmp_path / "lr"
    os.makedirs(hr)
    os.makedirs(lr)
    shutil.copy(str(pair_folders / "lr" / "b_one.png"), str(lr / "b_one.png"))
    _save(str(hr / "b_one.png"), _u8(0, 64, 60))
    from isr2_amd import cache
    with pytest.raises(ValueError, match="b_one.png"):
        cache.build_from_folders(model, str(hr), str(tmp_path / "out"), lr_dir=str(lr), patch=16, crops=1)
    assert cache.list_stems(str(tmp_path / "out")) == []


def test_build_from_folders_hr_only(model, tmp_path):
    from PIL import Image
    from isr2_amd import cache, ops
    hr_dir, out, lr_png = tmp_path / "hr", str(tmp_path / "out"), str(tmp_path / "lr_png")
    os.makedirs(hr_dir)
    images = (("m_odd", 94, 150), ("n_sq", 67, 66))                                        # cropped to 92x148 and 64x64: LR 23x37, 16x16
    for i, (stem, H, W) in enumerate(images):
        _save(str(hr_dir / f"{stem}.png"), _u8(30 + i, H, W))
    res = cache.build_from_folders(model, str(hr_dir), out, patch=16, crops=2, seed=1, write_lr=lr_png)
    assert res["images"] == 2 and res["images_skipped"] == 0 and res["patches_written"] == 4
    assert cache.list_stems(out) == ["m_odd_p0", "m_odd_p1", "n_sq_p0", "n_sq_p1"]
    want = {}
    for index, (stem, H, W) in enumerate(images):
        H4, W4 = H - H % 4, W - W % 4
        hr_u8 = torch.from_numpy(_u8(30 + index, H, W)[:H4, :W4].copy())
        lr_u8 = ops.f32_to_u8_image(ops.resize_aa(ops.u8_to_f32_image(hr_u8.cuda()), (H4 // 4, W4 // 4))).cpu()
        assert torch.equal(torch.from_numpy(np.array(Image.open(os.path.join(lr_png, stem + ".png")).convert("RGB"))), lr_u8)
        want[stem] = (lr_u8.permute(2, 0, 1).float() / 255.0, hr_u8.permute(2, 0, 1).float() / 255.0, H4 // 4, W4 // 4)
        for k, (t, l) in enumerate(cache.crop_plan(H4 // 4, W4 // 4, 16, 2, 1, index)):
            smp = cache.read_sample(out, f"{stem}_p{k}", load_features=False)
            assert torch.equal(smp["lr"], want[stem][0][:, t:t + 16, l:l + 16]), (stem, k)
            assert torch.equal(smp["hr"], want[stem][1][:, 4 * t:4 * t + 64, 4 * l:4 * l + 64]), (stem, k)
    # center=True: one pair of files per image, under the bare stem
    out_c = str(tmp_path / "out_center")
    res = cache.build_from_folders(model, str(hr_dir), out_c, patch=16, crops=2, seed=1, center=True)
    assert res["patches_written"] == 2 and cache.list_stems(out_c) == ["m_odd", "n_sq"]
    for stem, (lr, hr, h, w) in want.items():
        t, l = (h - 16) // 2, (w - 16) // 2
        smp = cache.read_sample(out_c, stem, load_features=False)
        assert torch.equal(smp["lr"], lr[:, t:t + 16, l:l + 16]) and torch.equal(smp["hr"], hr[:, 4 * t:4 * t + 64, 4 * l:4 * l + 64])


def test_build_from_folders_propagates_a_writer_failure(model, pair_folders, tmp_path, monkeypatch):
    from isr2_amd import cache
    real, calls = cache.write_sample, []

    def failing(cache_dir, stem, *a, **k):
        calls.append(stem)
        if len(calls) == 2:
            raise OSError("disk full (injected)")
        return real(cache_dir, stem, *a, **k)

    monkeypatch.setattr(cache, "write_sample", failing)
    out = str(tmp_path / "out")
    with pytest.raises(OSError, match="injected"):
        cache.build_from_folders(model, str(pair_folders / "hr"), out, lr_dir=str(pair_folders / "lr"), patch=16, crops=2, writers=1)
    names = os.listdir(out)
    for f in names:
        assert f.endswith(cache.PRIMARY_SUFFIX) or f.endswith(cache.REST_SUFFIX), f             # the temporary directory is gone
        if f.endswith(cache.PRIMARY_SUFFIX):
            assert f[:-len(cache.PRIMARY_SUFFIX)] + cache.REST_SUFFIX in names, f
    assert len(calls) >= 2 and len(cache.list_stems(out)) < 6
