"""ff_sample_pairs_u8 (csrc/sample_batch.hip, ops.sample_pairs_u8): one launch that crops, converts and augments a micro-batch out of a
packed pool of uint8 images.  Every case is torch.equal -- a permutation of exactly representable values, no tolerance -- against
two references: ops.d4_nchw(ops.crop_pairs_u8(...)), and a CPU restatement (uint8 slice -> / 255 in fp32 -> flip / rot90).
The pool holds LR images of 37x53, 64x64 and 70x41 with their 4x partners, packed back to back: odd bases, odd row pitches.  A fourth
image of 70x73 follows them: 70x41 cannot hold a 64x64 patch, so the full-tile case with an odd `left` is cut from that one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LR_SIZES = [(37, 53), (64, 64), (70, 41), (70, 73)]
ALL16 = list(range(16))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def pool():
    """(pool uint8 device tensor, [(lr_u8, hr_u8) host tensors], offsets int64 [n, 2]) -- built by hand, not by pool_layout."""
    _need_gpu()
    rng = np.random.default_rng(20260)
    imgs, offs, parts, n = [], [], [], 0
    for h, w in LR_SIZES:
        lr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        hr = rng.integers(0, 256, (4 * h, 4 * w, 3), dtype=np.uint8)
        offs.append((n, n + lr.size))
        n += lr.size + hr.size
        parts += [lr.reshape(-1), hr.reshape(-1)]
        imgs.append((torch.from_numpy(lr), torch.from_numpy(hr)))
    assert offs[1][0] % 2 == 1 and offs[2][1] % 2 == 1                  # odd bases
    return torch.from_numpy(np.concatenate(parts)).cuda(), imgs, np.array(offs, dtype=np.int64)


def _desc(offs, rows):
    """rows: (image, top, left, code) -> int64 [B, 8]."""
    return np.array([[offs[i][0], offs[i][1], LR_SIZES[i][0], LR_SIZES[i][1], t, l, c, 0] for i, t, l, c in rows], dtype=np.int64)


def _cpu_ref(imgs, rows, p):
    lrs, hrs = [], []
    for i, t, l, c in rows:
        pair = []
        for img, s in ((imgs[i][0], 1), (imgs[i][1], 4)):
            x = img[s * t:s * (t + p), s * l:s * (l + p)].permute(2, 0, 1).to(torch.float32) / 255.0
            if c & 1:
                x = torch.flip(x, dims=[-1])
            if c & 2:
                x = torch.flip(x, dims=[-2])
            if c >> 2:
                x = torch.rot90(x, k=c >> 2, dims=[-2, -1])
            pair.append(x.contiguous())
        lrs.append(pair[0])
        hrs.append(pair[1])
    return torch.stack(lrs), torch.stack(hrs)


def _kernel_ref(imgs, rows, p):
    """ops.d4_nchw(ops.crop_pairs_u8(...)), sample by sample (crop_pairs_u8 takes one image pair)."""
    from isr2_amd import ops
    lrs, hrs = [], []
    for i, t, l, c in rows:
        lr, hr = ops.crop_pairs_u8(imgs[i][0].cuda(), imgs[i][1].cuda(), [(t, l)], p)
        lrs.append(ops.d4_nchw(lr, [c]))
        hrs.append(ops.d4_nchw(hr, [c]))
    return torch.cat(lrs), torch.cat(hrs)


def _check(pool, rows, p, **kw):
    from isr2_amd import ops
    buf, imgs, offs = pool
    lr, hr = ops.sample_pairs_u8(buf, _desc(offs, rows), p, **kw)
    assert tuple(lr.shape) == (len(rows), 3, p, p) and tuple(hr.shape) == (len(rows), 3, 4 * p, 4 * p)
    rl, rh = _cpu_ref(imgs, rows, p)
    assert torch.equal(lr.cpu(), rl) and torch.equal(hr.cpu(), rh), (p, rows)
    kl, kh = _kernel_ref(imgs, rows, p)
    assert torch.equal(lr, kl) and torch.equal(hr, kh), (p, rows)
    return lr, hr


def _positions(p, n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for j in range(n):
        i = j % len(LR_SIZES)
        h, w = LR_SIZES[i]
        rows.append((i, int(rng.integers(0, h - p + 1)), int(rng.integers(0, w - p + 1))))
    return rows


@pytest.mark.parametrize("p", [6, 20])
def test_all_sixteen_codes(pool, p):
    """p = 6: p % 4 != 0, the dword form, HR 24.  p = 20: the float4 form; HR 80 = one full 64-tile and a clipped one in each axis,
    the LR patch smaller than a tile."""
    rows = [(i, t, l, c) for (i, t, l), c in zip(_positions(p, 16, p), ALL16)]
    assert any(l % 2 for _, _, l, _ in rows)
    _check(pool, rows, p)


def test_full_tiles_forced_origin_and_odd_left(pool):
    """p = 64: full tiles only, all 16 codes each.  The 64x64 image admits (0, 0) alone; the 70x73 image is cut at odd `left` values, its
    last row and column included.  70x41 (odd pitch, even base) is cut at p = 32 with an odd `left`."""
    _check(pool, [(1, 0, 0, c) for c in ALL16], 64)
    _check(pool, [(3, 3, 7, c) for c in ALL16], 64)
    _check(pool, [(3, 6, 9, c) for c in (0, 5, 10, 15)], 64)
    _check(pool, [(2, 38, 9, c) for c in ALL16], 32)
    _check(pool, [(2, 5, 7, c) for c in ALL16], 32)


def test_two_samples_of_one_image_and_the_last_row_and_column(pool):
    for p in (6, 20):
        h, w = LR_SIZES[0]
        rows = [(0, 0, 0, 5), (0, h - p, w - p, 5), (0, h - p, 0, 14), (0, 0, w - p, 7), (0, 3, 11, 0), (0, 3, 11, 9)]
        h2, w2 = LR_SIZES[2]
        rows += [(2, h2 - p, w2 - p, c) for c in (0, 3, 4, 13)]
        _check(pool, rows, p)


def test_outputs_and_descriptor_given_by_the_caller(pool):
    """out= tensors are filled in place, desc_dev= is used as it is; an unaligned out takes the dword form with the same bits."""
    from isr2_amd import ops
    buf, imgs, offs = pool
    p = 20
    rows = [(i, t, l, c) for (i, t, l), c in zip(_positions(p, 5, 99), (4, 1, 14, 8, 7))]
    d = _desc(offs, rows)
    lr0, hr0 = _check(pool, rows, p)
    flat_l, flat_h = torch.zeros(5 * 3 * p * p + 1, device="cuda"), torch.zeros(5 * 3 * 16 * p * p + 1, device="cuda")
    out = (flat_l[1:].view(5, 3, p, p), flat_h[1:].view(5, 3, 4 * p, 4 * p))
    lr, hr = ops.sample_pairs_u8(buf, d, p, desc_dev=torch.from_numpy(d).cuda(), out=out)
    assert lr.data_ptr() == out[0].data_ptr() and hr.data_ptr() == out[1].data_ptr() and lr.data_ptr() % 16 != 0
    assert torch.equal(lr, lr0) and torch.equal(hr, hr0)
    assert float(flat_l[0]) == 0.0 and float(flat_h[0]) == 0.0


def test_wrapper_refuses_before_any_launch(pool):
    from isr2_amd import lib as L
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    buf, imgs, offs = pool
    real, calls = L.load(), []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    p = 20
    h, w = LR_SIZES[0]
    good = _desc(offs, [(0, 1, 2, 3), (2, 4, 5, 6)])
    bad = []
    for col, val in ((5, w - p + 1), (4, h - p + 1), (4, -1), (5, -1), (6, 16), (6, -1), (0, buf.numel()), (1, buf.numel() - 48 * h * w + 1),
                     (0, -1), (2, 0)):
        d = good.copy()
        d[0, col] = val
        bad.append(d)
    L._lib = Spy()
    try:
        for d in bad:
            with pytest.raises(FFError):
                ops.sample_pairs_u8(buf, d, p)
        for args in ((buf, good[:0], p), (buf, good, 0), (buf, good[:, :7], p), (buf.view(1, -1), good, p), (buf.float(), good, p)):
            with pytest.raises(FFError):
                ops.sample_pairs_u8(*args)
        with pytest.raises(FFError):
            ops.sample_pairs_u8(buf, good, p, desc_dev=torch.from_numpy(good).cuda().to(torch.int32))
        with pytest.raises(FFError):
            ops.sample_pairs_u8(buf, good, p, out=(torch.zeros(2, 3, p, p, device="cuda"), torch.zeros(2, 3, p, p, device="cuda")))
    finally:
        L._lib = real
    assert "ff_sample_pairs_u8" not in calls
    _check(pool, [(0, 1, 2, 3), (2, 4, 5, 6)], p)                       # the table the bad ones were made from is fine
