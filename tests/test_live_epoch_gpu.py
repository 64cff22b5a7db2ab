"""Live-expert training on the GPU (isr2_amd.epoch: ImagePool, LiveEpoch, live_val_samples; train_epoch and fit over them): a folder of
five seeded PNG pairs (LR 24x40 ... 33x28) and one pair smaller than the patch; patch 16, B = 2, synthetic weights.  Everything is a
bit comparison: the pool against the decoded files, the micro-batches against a CPU restatement of live_plan and an eager expert
pass, an epoch over LiveEpoch against the same micro-batches handed over as a list, a resumed run against the uninterrupted one."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
EXPERTS = ("hat", "dat", "nafnet")
LR_SIZES = {"a0": (24, 40), "b1": (17, 31), "c2": (32, 16), "d3": (29, 23), "e4": (33, 28), "tiny": (12, 40)}
PATCH = 16


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _write_folders(root, sizes=LR_SIZES, seed=77):
    from PIL import Image
    rng = np.random.default_rng(seed)
    hr_dir, lr_dir = os.path.join(str(root), "hr"), os.path.join(str(root), "lr")
    os.makedirs(hr_dir)
    os.makedirs(lr_dir)
    imgs = {}
    for stem, (h, w) in sizes.items():
        # smooth-ish content: blocks of 4 so that the images are not pure noise, still every byte value
        lr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        hr = np.repeat(np.repeat(lr, 4, axis=0), 4, axis=1) ^ rng.integers(0, 32, (4 * h, 4 * w, 3), dtype=np.uint8)
        Image.fromarray(lr).save(os.path.join(lr_dir, stem + ".png"))
        Image.fromarray(hr).save(os.path.join(hr_dir, stem + ".png"))
        imgs[stem] = (torch.from_numpy(lr), torch.from_numpy(hr))
    return hr_dir, lr_dir, imgs


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    _need_gpu()
    return _write_folders(tmp_path_factory.mktemp("live"))


@pytest.fixture(scope="module")
def model(synth_sd):
    _need_gpu()
    from isr2_amd.model import FreqFusionHIP
    return FreqFusionHIP(synth_sd, "cuda:0")


@pytest.fixture(scope="module")
def pool(folders):
    from isr2_amd import epoch as E
    return E.ImagePool(folders[0], folders[1], patch=PATCH, readers=3)


def _d4(x, c):
    if c & 1:
        x = torch.flip(x, dims=[-1])
    if c & 2:
        x = torch.flip(x, dims=[-2])
    if c >> 2:
        x = torch.rot90(x, k=c >> 2, dims=[-2, -1])
    return x.contiguous()


def _restate(imgs, stems, plan, b, p=PATCH):
    """Micro-batch b of a live_plan, from the decoded files on the CPU."""
    idx, top, left, codes = plan
    lrs, hrs = [], []
    for j in range(idx.shape[1]):
        lr_u8, hr_u8 = imgs[stems[int(idx[b, j]) % len(stems)]]
        t, l, c = int(top[b, j]), int(left[b, j]), int(codes[b, j])
        lrs.append(_d4(lr_u8[t:t + p, l:l + p].permute(2, 0, 1).float() / 255.0, c))
        hrs.append(_d4(hr_u8[4 * t:4 * (t + p), 4 * l:4 * (l + p)].permute(2, 0, 1).float() / 255.0, c))
    return torch.stack(lrs), torch.stack(hrs)


def test_image_pool_holds_the_decoded_files(folders, pool):
    from isr2_amd import epoch as E
    from isr2_amd.lib import FFError
    hr_dir, lr_dir, imgs = folders
    assert pool.stems == ["a0", "b1", "c2", "d3", "e4"] and pool.skipped == 1 and len(pool) == 5
    assert pool.sizes == [LR_SIZES[s] for s in pool.stems]
    offs, total = E.pool_layout(pool.sizes)
    assert np.array_equal(offs, pool.offsets) and total == pool.total_bytes == pool.buf.numel()
    assert pool.buf.dtype == torch.uint8 and pool.buf.is_cuda
    host = pool.buf.cpu()
    want = torch.cat([t.reshape(-1) for s in pool.stems for t in imgs[s]])
    assert torch.equal(host, want)
    lr_v, hr_v = pool.image(3)
    assert torch.equal(lr_v.cpu(), imgs["d3"][0]) and torch.equal(hr_v.cpu(), imgs["d3"][1])
    # one byte too few is refused, naming both numbers; exactly enough is taken
    with pytest.raises(FFError) as ei:
        E.ImagePool(hr_dir, lr_dir, patch=PATCH, max_bytes=total - 1)
    assert str(total) in str(ei.value) and str(total - 1) in str(ei.value) and "max_bytes" in str(ei.value)
    assert E.ImagePool(hr_dir, lr_dir, patch=PATCH, max_bytes=total, readers=1).total_bytes == total
    with pytest.raises(FFError):
        E.ImagePool(hr_dir, lr_dir, patch=64)                           # no image holds the patch


def test_image_pool_refuses_a_pair_that_is_not_4x_and_a_missing_partner(tmp_path):
    _need_gpu()
    from PIL import Image
    from isr2_amd import epoch as E
    from isr2_amd.lib import FFError
    hr_dir, lr_dir, _ = _write_folders(tmp_path, {"ok": (20, 20), "odd": (18, 22)})
    Image.fromarray(np.zeros((72, 87, 3), dtype=np.uint8)).save(os.path.join(hr_dir, "odd.png"))      # 87 != 4 * 22
    with pytest.raises(FFError) as ei:
        E.ImagePool(hr_dir, lr_dir, patch=PATCH)
    assert "odd.png" in str(ei.value) and "72x87" in str(ei.value)
    os.remove(os.path.join(lr_dir, "odd.png"))
    with pytest.raises(FileNotFoundError):
        E.ImagePool(hr_dir, lr_dir, patch=PATCH)


def test_image_pool_hr_only_makes_lr_on_the_device(tmp_path):
    _need_gpu()
    from PIL import Image
    from isr2_amd import epoch as E
    from isr2_amd import ops
    rng = np.random.default_rng(5)
    hr_dir = str(tmp_path / "hr")
    os.makedirs(hr_dir)
    files = {"p": (97, 131), "q": (64, 64), "r": (70, 203), "small": (63, 200)}        # HR sizes, not multiples of 4
    for stem, (H, W) in files.items():
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(os.path.join(hr_dir, stem + ".png"))
    pool = E.ImagePool(hr_dir, None, patch=PATCH, readers=2)
    assert pool.stems == ["p", "q", "r"] and pool.skipped == 1 and pool.sizes == [(24, 32), (16, 16), (17, 50)]
    for i, stem in enumerate(pool.stems):
        h, w = pool.sizes[i]
        hr = torch.from_numpy(np.asarray(Image.open(os.path.join(hr_dir, stem + ".png")).convert("RGB"), dtype=np.uint8)[:4 * h, :4 * w].copy())
        lr = ops.f32_to_u8_image(ops.resize_aa(ops.u8_to_f32_image(hr.cuda()), (h, w)))
        lr_v, hr_v = pool.image(i)
        assert torch.equal(hr_v.cpu(), hr) and torch.equal(lr_v, lr), stem


def test_reader_exception_ends_construction(tmp_path):
    _need_gpu()
    from isr2_amd import epoch as E
    hr_dir, lr_dir, _ = _write_folders(tmp_path, {"a": (20, 20), "b": (18, 22), "c": (16, 16)})
    path = os.path.join(hr_dir, "b.png")
    blob = open(path, "rb").read()
    open(path, "wb").write(blob[:len(blob) // 2])                       # the header still reads, the pixel data is cut short
    with pytest.raises(Exception) as ei:
        E.ImagePool(hr_dir, lr_dir, patch=PATCH, readers=2)
    assert not isinstance(ei.value, (AssertionError, KeyboardInterrupt))


@pytest.mark.parametrize("overlap", [False, True])
def test_live_epoch_batches_are_the_plan_and_an_eager_expert_pass(folders, pool, model, overlap):
    from isr2_amd import epoch as E
    _, _, imgs = folders
    data = E.LiveEpoch(model, pool, batch_size=2, repeat_factor=2, augment=True, seed=11, overlap=overlap)
    try:
        assert len(data) == 5 and data.wait_s == 0.0
        kept = {}
        for epoch in (0, 1):
            plan = data.plan(epoch)
            want = E.live_plan(pool.sizes, 2, 2, PATCH, 11, epoch)
            assert all(np.array_equal(a, b) for a, b in zip(plan, want))
            n = 0
            for b, (lr, hr, outs, feats) in enumerate(data.batches(epoch)):
                rl, rh = _restate(imgs, pool.stems, plan, b)
                assert tuple(lr.shape) == (2, 3, 16, 16) and tuple(hr.shape) == (2, 3, 64, 64)
                assert torch.equal(lr.cpu(), rl) and torch.equal(hr.cpu(), rh), (epoch, b)
                eo, ef = model.experts_with_features(lr.clone())
                for k in EXPERTS:
                    assert tuple(outs[k].shape) == (2, 3, 64, 64) and tuple(feats[k].shape) == (2, 64 if k == "nafnet" else 180, 16, 16)
                    assert torch.equal(outs[k], eo[k]) and torch.equal(feats[k], ef[k]), (epoch, b, k)
                kept[epoch, b] = [t.clone() for t in (lr, hr, *outs.values(), *feats.values())]
                n += 1
            assert n == 5
        for b, (lr, hr, outs, feats) in enumerate(data.batches(0)):      # the same epoch again: the same bits
            assert all(torch.equal(a, c) for a, c in zip(kept[0, b], (lr, hr, *outs.values(), *feats.values())))
        assert any(not torch.equal(kept[0, b][0], kept[1, b][0]) for b in range(5))
        assert len({int(c) for e in range(4) for c in data.plan(e)[3].reshape(-1)}) > 4
    finally:
        data.close()
    plain = E.LiveEpoch(model, pool, batch_size=5, repeat_factor=1, augment=False, shuffle=False, overlap=overlap)
    try:
        (lr, hr, outs, feats), = list(plain.batches(0))
        rl, rh = _restate(imgs, pool.stems, plain.plan(0), 0)
        assert torch.equal(lr.cpu(), rl) and torch.equal(hr.cpu(), rh) and int(plain.plan(0)[3].max()) == 0
    finally:
        plain.close()
    with pytest.raises(Exception):
        next(plain.batches(0))                                          # closed


def test_overlap_yields_the_bits_of_the_single_lane(pool, model):
    """Two lanes with the next micro-batch's expert pass queued beside the consumer's work, against one lane on one stream; the consumer
    here queues real work on the asking stream between two micro-batches (a matrix product over the feature maps)."""
    from isr2_amd import epoch as E
    runs = {}
    for overlap in (False, True):
        data = E.LiveEpoch(model, pool, batch_size=2, repeat_factor=3, augment=True, seed=21, overlap=overlap)
        try:
            got = []
            for epoch in (0, 1):
                for lr, hr, outs, feats in data.batches(epoch):
                    busy = feats["hat"].reshape(2, 180, 256)
                    busy = torch.bmm(busy, busy.transpose(1, 2)).sum()             # reads the lane's buffers after the next replay was queued
                    got.append([t.clone() for t in (lr, hr, *outs.values(), *feats.values())] + [busy.clone()])
            it = data.batches(2)                                        # an abandoned epoch leaves the lanes usable
            next(it)
            it.close()
            got.append([t.clone() for t in next(iter(data.batches(0)))[:2]])
        finally:
            data.close()
        runs[overlap] = got
    assert len(runs[True]) == len(runs[False]) == 2 * 7 + 1
    for a, b in zip(runs[False], runs[True]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(runs[True][0], runs[True][14]))     # epoch 0's first micro-batch again


def _trainer(seed=5, dropout=0.1):
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    return FusionTrainer(synth_state_dict(1234, parts=("fusion", "collab")), "cuda:0", dropout=dropout, seed=seed)


def test_train_epoch_over_live_epoch_equals_the_same_micro_batches_as_a_list(pool, model):
    from isr2_amd import epoch as E
    data = E.LiveEpoch(model, pool, batch_size=2, repeat_factor=2, augment=True, seed=3)
    try:
        listed = [(lr.clone(), hr.clone(), {k: v.clone() for k, v in outs.items()}, {k: v.clone() for k, v in feats.items()})
                  for lr, hr, outs, feats in data.batches(0)]
        a, b = _trainer(), _trainer()
        ra = E.train_epoch(a, data, 0, accumulation_steps=2)
        rb = E.train_epoch(b, listed, 0, accumulation_steps=2)
    finally:
        data.close()
    assert (ra["micro_batches"], ra["optimizer_steps"], ra["discarded"]) == (5, 2, 1)
    assert ra["micro_losses"] == rb["micro_losses"] and all(math.isfinite(v) for v in ra["micro_losses"])
    assert torch.equal(a.P, b.P) and torch.equal(a.EMA, b.EMA)
    assert not torch.equal(a.P, _trainer().P)                           # the epoch did move the parameters


def test_fit_resumed_repeats_three_uninterrupted_epochs(folders, pool, model, tmp_path):
    from isr2_amd import epoch as E
    hr_dir, lr_dir, imgs = folders
    val = E.live_val_samples(model, hr_dir, lr_dir, patch=PATCH)
    assert [s["filename"] for s in val] == pool.stems and all("expert_feats" not in s for s in val)
    s = val[0]                                                          # the centre patch of the 24 x 40 image: (4, 12)
    assert torch.equal(s["lr"], imgs["a0"][0][4:20, 12:28].permute(2, 0, 1).float() / 255.0)
    assert torch.equal(s["hr"], imgs["a0"][1][16:80, 48:112].permute(2, 0, 1).float() / 255.0)
    eo, _ = model.experts_with_features(s["lr"][None].cuda())
    assert all(torch.equal(s["expert_imgs"][k], eo[k][0].cpu()) for k in EXPERTS)
    logs = {"a": [], "b": []}
    data = E.LiveEpoch(model, pool, batch_size=2, repeat_factor=1, augment=True, seed=9)
    try:
        a = _trainer()
        E.fit(a, data, val, str(tmp_path / "a"), epochs=3, accumulation_steps=2, log=logs["a"].append)
        b = _trainer()
        E.fit(b, data, val, str(tmp_path / "b"), epochs=2, accumulation_steps=2, log=logs["b"].append)
        c = _trainer(seed=0, dropout=0.0)
        ck = c.load_checkpoint(str(tmp_path / "b" / "latest.pth"))
        assert int(ck["epoch"]) == 1
        E.fit(c, data, val, str(tmp_path / "b"), epochs=3, start_epoch=int(ck["epoch"]) + 1, accumulation_steps=2, log=logs["b"].append)
    finally:
        data.close()
    rows_a, rows_b = ([json.loads(line) for line in logs[k]] for k in "ab")
    assert [r["epoch"] for r in rows_a] == [0, 1, 2] == [r["epoch"] for r in rows_b]
    for ra, rb in zip(rows_a, rows_b):
        assert ra["loss"] == rb["loss"] and ra["psnr"] == rb["psnr"] and ra["ssim"] == rb["ssim"] and ra["data_wait_s"] == 0.0
        assert ra["micro_batches"] == 2 and ra["optimizer_steps"] == 1 and math.isfinite(ra["psnr"])
    assert torch.equal(a.P, c.P) and torch.equal(a.EMA, c.EMA) and torch.equal(a.M, c.M) and torch.equal(a.V, c.V)
    assert a.step_count == c.step_count == 3


def test_train_live_command_runs_two_epochs_and_resumes(folders, tmp_path):
    hr_dir, lr_dir, _ = folders
    out = tmp_path / "run"
    cmd = [sys.executable, "-m", "isr2_amd.train_live", "--hr", hr_dir, "--lr", lr_dir, "--val-hr", hr_dir, "--val-lr", lr_dir, "--out", str(out),
           "--patch", "16", "--batch", "2", "--accum", "2", "--repeat", "2", "--expert-weights", str(tmp_path / "none"), "--readers", "2"]
    r = subprocess.run(cmd + ["--epochs", "2"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [row["epoch"] for row in rows] == [0, 1]
    for row in rows:
        assert all(math.isfinite(row[k]) for k in ("loss", "psnr", "ssim", "lr")), row
        assert row["micro_batches"] == 5 and row["optimizer_steps"] == 2 and row["discarded"] == 1 and row["stage"] == 1
    assert os.path.exists(out / "latest.pth") and os.path.exists(out / "best.pth")
    r = subprocess.run(cmd + ["--epochs", "3", "--resume"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [row["epoch"] for row in rows] == [2]
