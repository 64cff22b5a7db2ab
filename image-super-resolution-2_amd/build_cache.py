"""Build a cached-expert training set from image folders (the directory `python -m isr2_amd.train_cached --cache DIR` reads):

    python -m isr2_amd.build_cache --hr DIR [--lr DIR] --out DIR [--patch 64] [--crops 5] [--seed 0] [--center] [--write-lr DIR]
                                   [--weights PATH] [--pretrained DIR] [--gemm bf16x3] [--writers 4] [--batch 1] [--device cuda:0]

--hr / --lr: folders of images matched by stem; every HR image must be exactly 4x its LR partner.  Without --lr the LR images are
made on the device: HR cropped top-left to multiples of 4, antialiased bicubic x1/4, quantised to uint8 (--write-lr DIR keeps them as
PNGs).  --crops random patches per image (--center: the one centred patch) of --patch LR pixels go through the three frozen experts;
isr2_amd.cache.build_from_folders describes the files.  Expert weights come from where the plugin finds them: --pretrained DIR (default
$FREQFUSION_PRETRAINED, else ./pretrained) with hat/, dat/ and nafnet/ checkpoints; a missing one is replaced by seeded synthetic
weights with a warning (smoke runs).  --weights: a reference-keyed state dict, bare or under `model_state_dict`, laid over them as
train_cached lays it.  --batch N: the patches of an image go through the experts in groups of N (HAT, DAT and NAFNet batched: one launch per op); the
files hold the same bits.  One JSON line on stdout."""
from __future__ import annotations

import argparse
import json
import os
import sys
import warnings

import torch

EXPERT_FILES = {"hat": ("hat", "HAT-L_SRx4_ImageNet-pretrain.pth"), "dat": ("dat", "DAT_x4.pth"), "nafnet": ("nafnet", "NAFNet-SIDD-width64.pth")}


def load_state_dict(pretrained_dir: str, weights: str = None):
    """Seeded synthetic values first, then every tensor of the expert checkpoints and of `weights` whose name and shape match."""
    from .weights import synth_state_dict, param_spec, HAT_PREFIX, DAT_PREFIX, NAF_PREFIX
    sd = synth_state_dict(1234)
    shapes = {n: tuple(s) for n, s, _ in param_spec()}
    prefixes = {"hat": HAT_PREFIX, "dat": DAT_PREFIX, "nafnet": NAF_PREFIX}

    def overlay(src, prefix=""):
        n = 0
        for k, v in src.items():
            k = prefix + (k[len("module."):] if k.startswith("module.") else k)
            if k in shapes and tuple(v.shape) == shapes[k]:
                sd[k] = v.float()
                n += 1
        return n

    for name, (sub, fname) in EXPERT_FILES.items():
        path = os.path.join(pretrained_dir, sub, fname)
        if not os.path.exists(path):
            warnings.warn(f"{name} checkpoint not found: {path} -- using seeded synthetic weights")
            continue
        ck = torch.load(path, map_location="cpu", weights_only=True)
        for key in ("params_ema", "params", "state_dict", "model"):           # BasicSR-style containers
            if isinstance(ck, dict) and key in ck:
                ck = ck[key]
                break
        print(f"{name}: {overlay(ck, prefixes[name])} tensors from {path}", file=sys.stderr)
    if weights:
        ck = torch.load(weights, map_location="cpu", weights_only=True)
        n = overlay(ck.get("model_state_dict", ck) if isinstance(ck, dict) else ck)
        if n == 0:
            raise RuntimeError(f"{weights}: no tensor of the checkpoint matches the model")
        print(f"weights: {n} tensors from {weights}", file=sys.stderr)
    return sd


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m isr2_amd.build_cache", description=__doc__.split("\n\n")[0])
    ap.add_argument("--hr", required=True)
    ap.add_argument("--lr")
    ap.add_argument("--out", required=True)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--crops", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--center", action="store_true")
    ap.add_argument("--write-lr")
    ap.add_argument("--weights")
    ap.add_argument("--pretrained", default=os.environ.get("FREQFUSION_PRETRAINED", "pretrained"))
    ap.add_argument("--gemm", default="bf16x3", choices=("f32", "bf16", "bf16x2", "bf16x3"))
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    from . import cache, ops
    from .model import FreqFusionHIP
    ops.set_gemm_mode(a.gemm)
    model = FreqFusionHIP(load_state_dict(a.pretrained, a.weights), a.device)
    res = cache.build_from_folders(model, a.hr, a.out, lr_dir=a.lr, patch=a.patch, crops=a.crops, seed=a.seed, center=a.center,
                                   writers=a.writers, write_lr=a.write_lr, batch=a.batch)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
