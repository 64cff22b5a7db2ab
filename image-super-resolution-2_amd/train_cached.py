"""Fine-tune the fusion stack from a cached-expert directory with the reference's shipped configuration (configs/train_config.yaml:
AdamW 1.5e-4, warm-up 5 epochs + cosine restarts, batch 14, accumulation_steps 2, repeat_factor 20, EMA 0.9995, staged losses):

    python -m isr2_amd.train_cached --cache DIR --val-cache DIR --out DIR --epochs N [--resume PATH] [--weights PATH]
                                    [--batch 14] [--accum 2] [--repeat 20] [--validate-every 1] [--seed 0] [--no-augment]
                                    [--dropout 0.1] [--gemm f32] [--resident [--pool-gb 200] [--readers 8]]

The cache directories hold the two part files per sample that isr2_amd.cache.write_sample / extract (or the reference's own feature
extraction) write.  --weights: a reference-keyed fusion (+ collaborative) state dict, bare or under `model_state_dict`; without it
the seeded synthetic weights are used (smoke runs).  --resident: both caches are loaded once into device memory
(epoch.ResidentCache, --readers host threads, refused beyond --pool-gb GiB each) and every micro-batch is one gather launch
(epoch.ResidentEpoch): the same batches bit for bit, no file read after the load.  One JSON line per epoch on stdout; DIR/latest.pth after every
epoch, DIR/best.pth on a new best validation PSNR (EMA weights).  --resume continues at the checkpoint's epoch + 1."""
from __future__ import annotations

import argparse
import sys


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m isr2_amd.train_cached", description=__doc__.split("\n\n")[0])
    ap.add_argument("--cache", required=True)
    ap.add_argument("--val-cache", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--epochs", type=int, required=True)
    ap.add_argument("--resume")
    ap.add_argument("--weights")
    ap.add_argument("--batch", type=int, default=14)
    ap.add_argument("--accum", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--validate-every", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-augment", action="store_true")
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--gemm", default="f32", choices=("f32", "bf16x3"))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--pool-gb", type=float, default=200.0)
    ap.add_argument("--readers", type=int, default=8)
    a = ap.parse_args(argv)

    from . import epoch as E
    from .train import FusionTrainer, load_fusion_weights
    tr = FusionTrainer(load_fusion_weights(a.weights), a.device, dropout=a.dropout, seed=a.seed, gemm=a.gemm)
    start, best = 0, float("-inf")
    if a.resume:
        ck = tr.load_checkpoint(a.resume)
        start = int(ck["epoch"]) + 1
        best = float(ck.get("metrics", {}).get("best_psnr", best))
    if a.resident:
        cap = int(a.pool_gb * 2 ** 30)
        data = E.ResidentEpoch(E.ResidentCache(a.cache, a.device, a.readers, cap), a.batch, a.repeat, augment=not a.no_augment, seed=a.seed)
        val_pool = E.ResidentCache(a.val_cache, a.device, a.readers, cap)     # built once: validation reads no file either
        val = val_pool.samples
    else:
        data = E.CachedEpoch(a.cache, a.batch, a.repeat, augment=not a.no_augment, seed=a.seed, device=a.device)
        val = lambda: E.read_samples(a.val_cache)                     # noqa: E731
    E.fit(tr, data, val, a.out, a.epochs, start, a.accum, a.validate_every, best,
          log=lambda line: print(line, flush=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
