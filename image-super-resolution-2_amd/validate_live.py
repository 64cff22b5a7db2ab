"""Score checkpoints of a live (or cached) training run on one validation set, under the reference's own yardstick:

    python -m isr2_amd.validate_live --val-hr DIR [--val-lr DIR] --expert-weights DIR --ckpt A.pth [B.pth ...]
                                     [--protocol reference|patch] [--val-max-size 512] [--patch 64] [--no-ema]
                                     [--gemm f32] [--expert-gemm bf16x3] [--device cuda:0]

The set is built ONCE (the experts are frozen): --protocol reference (the default) is what the reference's train.py validates on --
every whole image pair, resized with OpenCV's INTER_CUBIC restated on the device when the LR's longer side exceeds
--val-max-size // 4 (epoch.live_val_images; 0 = no limit; the resize is parity unpinned (OpenCV absent)) --, --protocol patch the
centre --patch x --patch patches train_live validates on by default (epoch.live_val_samples).  Each checkpoint (the reference's
layout: train_live's latest.pth / best.pth) is loaded into a FusionTrainer and scored by epoch.validate with its EMA shadow (--no-ema:
its parameters).  One JSON line per checkpoint on stdout: {ckpt, psnr, ssim, images, skipped}.
Expert weights as in train_live: a missing checkpoint is replaced by seeded synthetic weights with a warning."""
from __future__ import annotations

import argparse
import json
import os
import sys


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m isr2_amd.validate_live", description=__doc__.split("\n\n")[0])
    ap.add_argument("--val-hr", required=True)
    ap.add_argument("--val-lr")
    ap.add_argument("--expert-weights", default=os.environ.get("FREQFUSION_PRETRAINED", "pretrained"))
    ap.add_argument("--ckpt", nargs="+", required=True)
    ap.add_argument("--protocol", default="reference", choices=("patch", "reference"))
    ap.add_argument("--val-max-size", type=int, default=512)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--no-ema", action="store_true")
    ap.add_argument("--gemm", default="f32", choices=("f32", "bf16x3"))
    ap.add_argument("--expert-gemm", default="bf16x3", choices=("f32", "bf16", "bf16x2", "bf16x3"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    from . import epoch as E
    from . import ops
    from .build_cache import load_state_dict
    from .model import FreqFusionHIP
    from .train import FusionTrainer, load_fusion_weights
    ops.set_gemm_mode(a.expert_gemm)
    model = FreqFusionHIP(load_state_dict(a.expert_weights), a.device)           # only its three experts run here
    if a.protocol == "reference":
        val = E.live_val_images(model, a.val_hr, a.val_lr, max_size=a.val_max_size if a.val_max_size > 0 else None)
    else:
        val = E.live_val_samples(model, a.val_hr, a.val_lr, patch=a.patch)
    tr = FusionTrainer(load_fusion_weights(None), a.device, dropout=0.0, gemm=a.gemm)
    for path in a.ckpt:
        tr.load_checkpoint(path)
        m = E.validate(tr, val, use_ema=not a.no_ema)
        print(json.dumps(dict(ckpt=path, psnr=m["psnr"], ssim=m["ssim"], images=len(val), skipped=int(getattr(val, "skipped", 0)))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
