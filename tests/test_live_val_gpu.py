"""The reference's validation protocol on the GPU (isr2_amd.epoch.live_val_images, fit(validate_start=...), train_live --val-protocol,
isr2_amd.validate_live): whole images, resized with OpenCV's INTER_CUBIC restated when the LR's longer side exceeds max_size // 4,
against validate_live_ms64.npz -- the reference's own validate_epoch(cached_mode=False) with EMA weights on three seeded pairs -- and
through the two command lines on a four-image folder."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)

import cv_cubic_ref as R  # noqa: E402

EXPERTS = ("hat", "dat", "nafnet")
EVAL_BARS = {"f32": 5e-5, "bf16x3": 2e-4}                              # tests/test_epoch_gpu.py, test_validate_against_reference
# LR sizes; max_size 64 resizes the first three to 9 x 16, 10 x 16 and 16 x 9 (DAT's reflect pad to 16 needs a side of 9 or more, as in torch)
FOLDER = {"a0": (24, 40), "b1": (20, 31), "c2": (28, 16), "d3": (16, 16)}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _write_pairs(root, pairs):
    from PIL import Image
    hr_dir, lr_dir = os.path.join(str(root), "hr"), os.path.join(str(root), "lr")
    os.makedirs(hr_dir)
    os.makedirs(lr_dir)
    for stem, (lr, hr) in pairs.items():
        Image.fromarray(lr).save(os.path.join(lr_dir, stem + ".png"))
        Image.fromarray(hr).save(os.path.join(hr_dir, stem + ".png"))
    return hr_dir, lr_dir


def _seeded_pairs(sizes, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for stem, (h, w) in sizes.items():
        lr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out[stem] = (lr, np.repeat(np.repeat(lr, 4, axis=0), 4, axis=1) ^ rng.integers(0, 32, (4 * h, 4 * w, 3), dtype=np.uint8))
    return out


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(GOLD, "validate_live_ms64.npz"))
    return g, json.loads(str(g["meta"]))


@pytest.fixture(scope="module")
def model(synth_sd):
    _need_gpu()
    from isr2_amd.model import FreqFusionHIP
    return FreqFusionHIP(synth_sd, "cuda:0")


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_live_val_images_and_validate_against_the_reference(gold, model, tmp_path, mode):
    """live_val_images' lr / hr are the restatement's bits; validate() on them with the EMA shadow against the reference's validate_epoch.
    Bars as tests/test_epoch_gpu.py::test_validate_against_reference: |sr - ref| < EVAL_BARS[mode], PSNR within
    20 log10(1 + bar / rmse_ref), the metrics within 2e-4 dB / 2e-6 of the oracle's on the same SR."""
    from isr2_amd import epoch as E
    from isr2_amd import ops
    from isr2_amd.train import FusionTrainer, to_native
    from isr2_amd.weights import synth_state_dict
    from oracle import freqfusion_oracle as O
    g, meta = gold
    bar = EVAL_BARS[mode]
    pairs = {s: (g["lr_u8/" + s], g["hr_u8/" + s]) for s in meta["stems"]}
    hr_dir, lr_dir = _write_pairs(tmp_path, pairs)
    extra = _seeded_pairs({"odd": (10, 10)}, 3)["odd"]                  # a pair whose HR is not 4x its LR: left out and counted
    from PIL import Image
    Image.fromarray(extra[0]).save(os.path.join(lr_dir, "odd.png"))
    Image.fromarray(extra[1][:39]).save(os.path.join(hr_dir, "odd.png"))
    old = ops.gemm_mode()
    ops.set_gemm_mode(mode)                                             # the experts' contraction mode
    try:
        samples = E.live_val_images(model, hr_dir, lr_dir, max_size=meta["max_size"])
        whole = E.live_val_images(model, hr_dir, lr_dir, max_size=None)
        eo, _ = model.experts_with_features(samples[0]["lr"][None].cuda())
    finally:
        ops.set_gemm_mode(old)
    assert [s["filename"] for s in samples] == meta["stems"] and samples.skipped == 1 and whole.skipped == 1
    assert all("expert_feats" not in s and set(s) == {"lr", "hr", "expert_imgs", "filename"} for s in samples)
    for s, w in zip(samples, whole):
        lr_u8, hr_u8 = pairs[s["filename"]]
        lr, hr = R.val_pair(lr_u8, hr_u8, max_size=meta["max_size"])
        assert list(lr.shape[-2:]) == meta["lr_shapes"][s["filename"]]
        assert torch.equal(s["lr"], torch.from_numpy(lr)) and torch.equal(s["hr"], torch.from_numpy(hr)), s["filename"]
        assert all(tuple(s["expert_imgs"][k].shape) == tuple(s["hr"].shape) for k in EXPERTS)
        assert torch.equal(w["lr"], torch.from_numpy(lr_u8).permute(2, 0, 1).float() / 255.0)      # max_size None: the decoded image
        assert torch.equal(w["hr"], torch.from_numpy(hr_u8).permute(2, 0, 1).float() / 255.0)
    assert all(torch.equal(samples[0]["expert_imgs"][k], eo[k][0].cpu()) for k in EXPERTS)
    assert torch.equal(samples[2]["lr"], whole[2]["lr"]) and not samples[0]["lr"].shape == whole[0]["lr"].shape

    tr = FusionTrainer(synth_state_dict(meta["weight_seed"], parts=("fusion", "collab")), "cuda:0", dropout=0.0, gemm=mode)
    other = synth_state_dict(meta["ema_seed"], parts=("fusion", "collab"))
    assert len(tr.names) == meta["shadow_taken"]
    for k in tr.names:
        tr.EMA[tr.offs[k]:tr.offs[k] + other[k].numel()].copy_(to_native(k, other[k].float()).reshape(-1))
    r = E.validate(tr, samples, use_ema=True, return_sr=True)
    ps, ss = [], []
    for b, s in enumerate(samples):
        ref = torch.from_numpy(g["sr/" + s["filename"]])
        d = float((r["sr"][b] - ref).abs().max())
        pb, sb = (float(v) for v in g["per_image"][b])
        print(mode, s["filename"], "max |sr - ref| =", d, "PSNR / SSIM", r["per_image"][b], "ref", (pb, sb))
        ps.append(O.metric_psnr(r["sr"][b][None], s["hr"][None].clamp(0, 1), 4, True))
        ss.append(O.metric_ssim(r["sr"][b][None], s["hr"][None].clamp(0, 1), 4, True))
    ref_psnr, ref_ssim = (float(v) for v in g["mean"])
    bound = 20 * math.log10(1 + bar / 10 ** (-ref_psnr / 20))
    print(mode, "PSNR", r["psnr"], "ref", ref_psnr, "bound", bound, "SSIM", r["ssim"], "ref", ref_ssim)
    for b, s in enumerate(samples):
        assert float((r["sr"][b] - torch.from_numpy(g["sr/" + s["filename"]])).abs().max()) < bar, s["filename"]
        assert abs(r["per_image"][b][0] - ps[b]) < 2e-4 and abs(r["per_image"][b][1] - ss[b]) < 2e-6
        pb = float(g["per_image"][b][0])
        assert abs(r["per_image"][b][0] - pb) < 20 * math.log10(1 + bar / 10 ** (-pb / 20))
    assert abs(r["psnr"] - float(np.mean(ps))) < 2e-4 and abs(r["ssim"] - float(np.mean(ss))) < 2e-6
    assert abs(r["psnr"] - ref_psnr) < bound
    assert abs(r["psnr"] - meta["mean_without_ema"][0]) > 0.1          # the shadow is what was evaluated


def test_fit_validates_from_validate_start_and_in_the_last_epoch(tmp_path):
    """fit's rule on the host side of its loop: which epochs carry metrics (a stub trainer: no GPU work, but fit synchronises the device)."""
    _need_gpu()
    from isr2_amd import epoch as E

    class Stub:
        dev, hp = torch.device("cuda:0"), {"lr": 1e-4}

        def save_checkpoint(self, path, **kw):
            open(path, "wb").write(b"x")
    real_train, real_val = E.train_epoch, E.validate
    E.train_epoch = lambda *a, **k: {"loss": 1.0}
    E.validate = lambda *a, **k: {"psnr": 20.0, "ssim": 0.5}
    try:
        def epochs_validated(**kw):
            rows = []
            E.fit(Stub(), [], [], str(tmp_path / "o"), log=rows.append, **kw)
            return [json.loads(r)["epoch"] for r in rows if "psnr" in json.loads(r)]
        assert epochs_validated(epochs=4) == [0, 1, 2, 3]                                           # the default: unchanged
        assert epochs_validated(epochs=4, validate_start=2) == [2, 3]
        assert epochs_validated(epochs=4, validate_start=9) == [3]                                  # always the last epoch
        assert epochs_validated(epochs=6, validate_every=2, validate_start=2) == [3, 5]             # (epoch + 1) % 2 == 0 is kept
        assert epochs_validated(epochs=5, validate_every=2, validate_start=0) == [1, 3, 4]
    finally:
        E.train_epoch, E.validate = real_train, real_val


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """train_live twice on a four-image folder: two epochs under the reference protocol, one under the default patch protocol."""
    _need_gpu()
    root = tmp_path_factory.mktemp("val_live")
    hr_dir, lr_dir = _write_pairs(root, _seeded_pairs(FOLDER, 78))
    base = [sys.executable, "-m", "isr2_amd.train_live", "--hr", hr_dir, "--lr", lr_dir, "--val-hr", hr_dir, "--val-lr", lr_dir, "--patch", "16",
            "--batch", "2", "--accum", "2", "--repeat", "1", "--expert-weights", str(root / "none"), "--readers", "2"]
    out = {"hr": hr_dir, "lr": lr_dir, "none": str(root / "none")}
    for tag, extra in (("reference", ["--val-protocol", "reference", "--val-max-size", "64", "--validate-start", "1", "--epochs", "2"]),
                       ("patch", ["--val-protocol", "patch", "--epochs", "1"])):
        r = subprocess.run(base + ["--out", str(root / tag)] + extra, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        out[tag] = (str(root / tag), [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")])
    return out


def _direct(model, ckpt, samples):
    from isr2_amd import epoch as E
    from isr2_amd.train import FusionTrainer, load_fusion_weights
    tr = FusionTrainer(load_fusion_weights(None), "cuda:0", dropout=0.0)
    tr.load_checkpoint(ckpt)
    return E.validate(tr, samples, use_ema=True)


def test_train_live_reference_protocol_validates_from_validate_start(runs, model):
    from isr2_amd import epoch as E
    out, rows = runs["reference"]
    assert os.path.exists(os.path.join(out, "latest.pth")) and os.path.exists(os.path.join(out, "best.pth"))
    assert [r["epoch"] for r in rows] == [0, 1]
    assert "psnr" not in rows[0] and "ssim" not in rows[0] and "best" not in rows[0]
    assert math.isfinite(rows[1]["psnr"]) and math.isfinite(rows[1]["ssim"]) and rows[1]["best"] is True
    samples = E.live_val_images(model, runs["hr"], runs["lr"], max_size=64)
    assert [tuple(s["lr"].shape[-2:]) for s in samples] == [(9, 16), (10, 16), (16, 9), (16, 16)]
    m = _direct(model, os.path.join(out, "latest.pth"), samples)
    assert (m["psnr"], m["ssim"]) == (rows[1]["psnr"], rows[1]["ssim"])  # the logged line is this set's score, bit for bit


def test_train_live_patch_protocol_is_live_val_samples(runs, model):
    from isr2_amd import epoch as E
    out, rows = runs["patch"]
    assert [r["epoch"] for r in rows] == [0] and math.isfinite(rows[0]["psnr"])
    m = _direct(model, os.path.join(out, "latest.pth"), E.live_val_samples(model, runs["hr"], runs["lr"], patch=16))
    assert (m["psnr"], m["ssim"]) == (rows[0]["psnr"], rows[0]["ssim"])
    ref = _direct(model, os.path.join(out, "latest.pth"), E.live_val_images(model, runs["hr"], runs["lr"], max_size=64))
    assert ref["psnr"] != m["psnr"]                                     # the two protocols score different things


def test_validate_live_prints_one_line_per_checkpoint(runs, model):
    from isr2_amd import epoch as E
    a, b = os.path.join(runs["reference"][0], "latest.pth"), os.path.join(runs["patch"][0], "latest.pth")
    cmd = [sys.executable, "-m", "isr2_amd.validate_live", "--val-hr", runs["hr"], "--val-lr", runs["lr"], "--expert-weights", runs["none"],
           "--ckpt", a, b, "--protocol", "reference", "--val-max-size", "64"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [row["ckpt"] for row in rows] == [a, b] and all(set(row) == {"ckpt", "psnr", "ssim", "images", "skipped"} for row in rows)
    assert all(row["images"] == 4 and row["skipped"] == 0 for row in rows)
    samples = E.live_val_images(model, runs["hr"], runs["lr"], max_size=64)
    m = _direct(model, a, samples)
    assert rows[0]["psnr"] == m["psnr"] and rows[0]["ssim"] == m["ssim"]
    assert rows[0]["psnr"] == runs["reference"][1][1]["psnr"]           # and what train_live logged for that epoch
    assert rows[1]["psnr"] != rows[0]["psnr"]
