"""Fixture of LIVE validation on whole images -- the reference's own validate_epoch (train.py:413-523, cached_mode=False: model(lr)
with the three experts run on every image, EMA weights applied) --, generated from the IMPORTED reference (build container only; the
reference's code never leaves it -- only the arrays below are committed).  Run on the CPU:

    python tests/golden/make_golden_val_live.py        # validate_live_ms64.npz   (about three minutes)

What is run:
    model = CompleteEnhancedFusionSR(expert_ensemble=ExpertEnsemble(...), ...)            # _ref_import.build_reference_model
    weights: isr2_amd.weights.synth_state_dict(1234), all five parts; EMA shadow overwritten with synth_state_dict(4321)'s values for
             every shadow tensor that dict holds (as make_golden_epoch.py validate), so that the shadow is what gets evaluated
    loader:  a plain list of {'lr' [1,3,h,w], 'hr' [1,3,4h,4w], 'filename'} WHOLE images -- what ValidationDataset(max_size=64) yields
             (dataset.py:473-506) for three seeded uint8 pairs, with its two cv2.resize calls replaced by the fp32 restatement of
             INTER_CUBIC in cv_cubic_ref.py (OpenCV is not installed; parity with an OpenCV binary is unpinned):
                 a  LR 40x24 -> 16x9, HR 64x36     the height branch; neither side a multiple of the experts' windows
                 b  LR 12x20 ->  9x16, HR 36x64    the width branch (20 > 64 // 4, so this one is resized too)
                 c  LR 12x16 kept,     HR 48x64    max(h, w) == 64 // 4: no resize
    validate_epoch(model, loader, cpu, 0, {'validation': {crop_border 4, test_y_channel True}}, ema=ema, cached_mode=False)

Stored: the uint8 inputs, per image PSNR / SSIM (src.utils.metrics on the clamped SR of a second, identical pass with the shadow
applied), validate_epoch's means, the clamped SR.  Nothing of the reference's text."""
import contextlib
import io as _io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from _ref_import import build_reference_model  # noqa: E402
import cv_cubic_ref as R  # noqa: E402
from isr2_amd.weights import synth_state_dict  # noqa: E402

NAME, MAX_SIZE, WEIGHT_SEED, EMA_SEED, INPUT_SEED = "validate_live_ms64", 64, 1234, 4321, 641
LR_SIZES = {"a": (40, 24), "b": (12, 20), "c": (12, 16)}


def make_pairs(seed=INPUT_SEED, sizes=LR_SIZES):
    """{stem: (lr_u8 [h,w,3], hr_u8 [4h,4w,3])}: LR bytes, HR = the LR in 4x4 blocks with its five low bits redrawn."""
    rng = np.random.default_rng(seed)
    out = {}
    for stem, (h, w) in sizes.items():
        lr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        hr = np.repeat(np.repeat(lr, 4, axis=0), 4, axis=1) ^ rng.integers(0, 32, (4 * h, 4 * w, 3), dtype=np.uint8)
        out[stem] = (lr, hr)
    return out


def main():
    torch.manual_seed(0)
    model, ens = build_reference_model()
    res = model.load_state_dict(synth_state_dict(WEIGHT_SEED, parts=("hat", "dat", "nafnet", "fusion", "collab")), strict=False)
    assert not res.unexpected_keys, res.unexpected_keys[:5]
    with contextlib.redirect_stdout(_io.StringIO()):
        from src.utils.checkpoint_manager import EMAModel
        from src.utils.metrics import calculate_psnr, calculate_ssim
        from train import validate_epoch
    ema = EMAModel(model, decay=0.9995)
    other = synth_state_dict(EMA_SEED, parts=("fusion", "collab"))
    taken = [k for k in ema.shadow if k in other]
    for k in taken:
        assert tuple(other[k].shape) == tuple(ema.shadow[k].shape), k
        ema.shadow[k] = other[k].float().clone()
    pairs = make_pairs()
    loader, blob = [], {}
    for stem, (lr_u8, hr_u8) in pairs.items():
        lr, hr = R.val_pair(lr_u8, hr_u8, max_size=MAX_SIZE)
        loader.append({"lr": torch.from_numpy(lr)[None], "hr": torch.from_numpy(hr)[None], "filename": stem + ".png"})
        blob["lr_u8/" + stem], blob["hr_u8/" + stem] = lr_u8, hr_u8
    shapes = {b["filename"][:-4]: list(b["lr"].shape[-2:]) for b in loader}
    assert shapes == {"a": [16, 9], "b": [9, 16], "c": [12, 16]}, shapes
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with contextlib.redirect_stderr(_io.StringIO()):
        means = validate_epoch(model, loader, torch.device("cpu"), 0, {"validation": {"crop_border": 4, "test_y_channel": True}}, ema=ema,
                               cached_mode=False)
        means_off = validate_epoch(model, loader, torch.device("cpu"), 0, {"validation": {"crop_border": 4, "test_y_channel": True}}, ema=None,
                                   cached_mode=False)
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    per = []
    with torch.no_grad():
        model.eval()
        backup = ema.save(model)
        ema.apply(model)
        for b in loader:
            sr = model(b["lr"]).clamp(0, 1)
            per.append((calculate_psnr(sr[0], b["hr"][0], 4, True), calculate_ssim(sr[0], b["hr"][0], 4, True)))
            blob["sr/" + b["filename"][:-4]] = sr[0].numpy().astype(np.float32)
        ema.restore(model, backup)
    per = np.array(per, dtype=np.float64)
    assert abs(per[:, 0].mean() - means["psnr"]) < 1e-9 and abs(per[:, 1].mean() - means["ssim"]) < 1e-12, (per, means)
    assert abs(means["psnr"] - means_off["psnr"]) > 0.1, (means, means_off)                     # or the shadow proves nothing
    blob["meta"] = np.array(json.dumps({"max_size": MAX_SIZE, "weight_seed": WEIGHT_SEED, "ema_seed": EMA_SEED, "input_seed": INPUT_SEED,
                                        "stems": list(pairs), "lr_shapes": shapes, "crop_border": 4, "test_y_channel": True,
                                        "shadow_taken": len(taken), "mean_without_ema": [means_off["psnr"], means_off["ssim"]]}))
    blob["per_image"] = per
    blob["mean"] = np.array([means["psnr"], means["ssim"]], dtype=np.float64)
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **blob)
    print("wrote", NAME + ".npz", os.path.getsize(path) // 1024, "KiB;", len(taken), "of", len(ema.shadow), "shadow tensors replaced; EMA on", means,
          "off", means_off, "per image", per.tolist(), flush=True)
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("FF_THREADS", "8")))
    main()
