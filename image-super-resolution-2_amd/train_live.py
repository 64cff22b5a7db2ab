"""Fine-tune the fusion stack from image folders with the three frozen experts run on every micro-batch -- the reference's default
training (train.py:130-250 train_epoch; configs/train_config.yaml: dataset.train.cache_data false, repeat_factor 6, AdamW 1.5e-4,
warm-up 5 epochs + cosine restarts, batch 14, accumulation_steps 2, EMA 0.9995, staged losses):

    python -m isr2_amd.train_live --hr DIR [--lr DIR] --val-hr DIR [--val-lr DIR] --out DIR --epochs N [--resume] [--weights PATH]
                                  [--expert-weights DIR] [--batch 14] [--accum 2] [--repeat 6] [--patch 64] [--validate-every 1]
                                  [--seed 0] [--no-augment] [--dropout 0.1] [--gemm f32] [--expert-gemm bf16x3] [--readers 8]
                                  [--pool-gb 64] [--device cuda:0] [--color-jitter] [--jitter-prob 0.5] [--jitter-range 0.2 0.2 0.2]
                                  [--val-protocol patch|reference] [--val-max-size 512] [--validate-start 0]

--hr / --lr: folders of images matched by stem, every HR image exactly 4x its LR partner; without --lr the LR images are made on the
device (antialiased bicubic x1/4 of the HR image cropped to multiples of 4, quantised to uint8).  The training images are decoded once
into a device-resident pool (isr2_amd.epoch.ImagePool; more than --pool-gb GiB is an error); every epoch cuts fresh random crops with
paired flips / rotations out of it (epoch.live_plan, one sampler launch per micro-batch) and replays the expert graph on them
(epoch.LiveEpoch).  The validation set is the centre patch of every --val-hr image, its expert outputs computed once
(--val-protocol patch, the default: epoch.live_val_samples) or, with --val-protocol reference, what the reference's train.py validates
on: every whole --val-hr / --val-lr pair, resized with OpenCV's INTER_CUBIC restated on the device when the LR's longer side exceeds
--val-max-size // 4 (epoch.live_val_images; 0 = no limit; the resize is parity unpinned (OpenCV absent)).  --validate-start N: no
validation before epoch N, the last epoch excepted.
Expert weights: --expert-weights DIR (default $FREQFUSION_PRETRAINED, else ./pretrained) with hat/, dat/ and nafnet/ checkpoints as
the plugin finds them; a missing one is replaced by seeded synthetic weights with a warning (smoke runs).  --weights: a
reference-keyed fusion (+ collaborative) state dict, bare or under `model_state_dict`; without it the seeded synthetic weights.
--expert-gemm is the experts' contraction mode, --gemm the trainer's.  One JSON line per epoch on stdout; DIR/latest.pth after every
epoch, DIR/best.pth on a new best validation PSNR (EMA weights).  --resume continues at the epoch after DIR/latest.pth's.
--color-jitter: the reference's paired colour jitter on the device (augmentations.py:207-264; epoch.live_jitter_plan, two launches per
micro-batch between the sampler and the experts, csrc/color_jitter.hip): with probability --jitter-prob a sample's LR and HR patch get
brightness, contrast and saturation factors 1 + uniform(-r, r), r = --jitter-range B C S.  The defaults are the values the reference
trains with (its class defaults; the YAML's are never read).  Off unless asked for; validation samples are never jittered.  Its
draws are parity unpinned (RNG stream), its 8-bit HSV step parity unpinned (OpenCV absent).
Not applied: the reference's OpenCV resize of TRAINING images smaller than the patch (the pool holds uint8), SyncBatchNorm / several GPUs."""
from __future__ import annotations

import argparse
import os
import sys


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m isr2_amd.train_live", description=__doc__.split("\n\n")[0])
    ap.add_argument("--hr", required=True)
    ap.add_argument("--lr")
    ap.add_argument("--val-hr", required=True)
    ap.add_argument("--val-lr")
    ap.add_argument("--out", required=True)
    ap.add_argument("--epochs", type=int, required=True)
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--weights")
    ap.add_argument("--expert-weights", default=os.environ.get("FREQFUSION_PRETRAINED", "pretrained"))
    ap.add_argument("--batch", type=int, default=14)
    ap.add_argument("--accum", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=6)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--validate-every", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-augment", action="store_true")
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--gemm", default="f32", choices=("f32", "bf16x3"))
    ap.add_argument("--expert-gemm", default="bf16x3", choices=("f32", "bf16", "bf16x2", "bf16x3"))
    ap.add_argument("--readers", type=int, default=8)
    ap.add_argument("--pool-gb", type=float, default=64.0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--color-jitter", action="store_true")
    ap.add_argument("--jitter-prob", type=float, default=0.5)
    ap.add_argument("--jitter-range", type=float, nargs=3, default=[0.2, 0.2, 0.2], metavar=("B", "C", "S"))
    ap.add_argument("--val-protocol", default="patch", choices=("patch", "reference"))
    ap.add_argument("--val-max-size", type=int, default=512)
    ap.add_argument("--validate-start", type=int, default=0)
    a = ap.parse_args(argv)

    from . import epoch as E
    from . import ops
    from .build_cache import load_state_dict
    from .model import FreqFusionHIP
    from .train import FusionTrainer, load_fusion_weights
    ops.set_gemm_mode(a.expert_gemm)
    model = FreqFusionHIP(load_state_dict(a.expert_weights), a.device)           # only its three experts run here
    tr = FusionTrainer(load_fusion_weights(a.weights), a.device, dropout=a.dropout, seed=a.seed, gemm=a.gemm)
    start, best = 0, float("-inf")
    if a.resume:
        ck = tr.load_checkpoint(os.path.join(a.out, "latest.pth"))
        start = int(ck["epoch"]) + 1
        best = float(ck.get("metrics", {}).get("best_psnr", best))
    if a.val_protocol == "reference":
        val = E.live_val_images(model, a.val_hr, a.val_lr, max_size=a.val_max_size if a.val_max_size > 0 else None)
    else:
        val = E.live_val_samples(model, a.val_hr, a.val_lr, patch=a.patch)
    pool = E.ImagePool(a.hr, a.lr, patch=a.patch, device=a.device, readers=a.readers, max_bytes=int(a.pool_gb * (1 << 30)))
    jitter = dict(prob=a.jitter_prob, brightness=a.jitter_range[0], contrast=a.jitter_range[1], saturation=a.jitter_range[2]) if a.color_jitter else None
    data = E.LiveEpoch(model, pool, a.batch, a.repeat, augment=not a.no_augment, seed=a.seed, color_jitter=jitter)
    try:
        E.fit(tr, data, val, a.out, a.epochs, start, a.accum, a.validate_every, best, log=lambda line: print(line, flush=True),
              validate_start=a.validate_start)
    finally:
        data.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
