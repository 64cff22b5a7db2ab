"""Time one whole training epoch from a cache directory on one MI355X: N synthetic samples (tests/golden/train_inputs.make_train_batch)
are written to a temporary cache, one epoch runs through isr2_amd.epoch (reader thread -> pinned slot -> one upload -> ff_d4_nchw ->
accumulated steps), and samples/s plus the share of wall time the stepping thread waited for data are printed.
    python tools/epoch_bench.py [--samples 256] [--size 64] [--batch 14] [--accum 2] [--mode f32] [--d4-only]
--d4-only: time the eight augmentation launches of one micro-batch alone (under rocprofv3 --kernel-trace --stats the per-kernel
table comes out of the same command) and print the GB/s of the largest tensor."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=14)
    ap.add_argument("--accum", type=int, default=2)
    ap.add_argument("--mode", default="f32")
    ap.add_argument("--d4-only", action="store_true")
    a = ap.parse_args()
    from train_inputs import make_train_batch
    from isr2_amd import cache, ops
    from isr2_amd import epoch as E
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    if a.d4_only:
        B, s = a.batch, a.size
        shapes = [(B, 3, s, s)] + [(B, 3, 4 * s, 4 * s)] * 4 + [(B, 180, s, s)] * 2 + [(B, 64, s, s)]
        xs = [torch.randn(sh, device="cuda") for sh in shapes]
        outs = [torch.empty_like(x) for x in xs]
        codes = [i % 16 for i in range(B)]
        cd = torch.tensor(codes, dtype=torch.int32).cuda()
        for rep in range(3):
            for x, o in zip(xs, outs):
                ops.d4_nchw(x, codes, out=o, codes_dev=cd)
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        n = 20
        e0.record()
        for _ in range(n):
            for x, o in zip(xs, outs):
                ops.d4_nchw(x, codes, out=o, codes_dev=cd)
        e1.record()
        for _ in range(n):
            ops.d4_nchw(xs[5], codes, out=outs[5], codes_dev=cd)
        e2.record()
        torch.cuda.synchronize()
        ms_all, ms_feat = e0.elapsed_time(e1) / n, e1.elapsed_time(e2) / n
        nbytes = sum(x.numel() for x in xs) * 8
        print(json.dumps({"d4_micro_batch_ms": ms_all, "micro_batch_GBps": nbytes / ms_all / 1e6, "feat_shape": list(shapes[5]),
                          "feat_ms": ms_feat, "feat_GBps": xs[5].numel() * 8 / ms_feat / 1e6, "codes": "all 16 mixed"}), flush=True)
        return
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        done = 0
        while done < a.samples:
            nb = min(16, a.samples - done)
            d = {k: torch.from_numpy(v) for k, v in make_train_batch(7000 + done, nb, a.size, a.size).items()}
            for j in range(nb):
                cache.write_sample(tmp, f"s{done + j:05d}", d["lr"][j], d["hr"][j], {k: d["out_" + k][j:j + 1] for k in E.EXPERTS},
                                   {k: d["feat_" + k][j:j + 1] for k in E.EXPERTS})
            done += nb
        t_write = time.perf_counter() - t0
        tr = FusionTrainer(synth_state_dict(1234, parts=("fusion", "collab")), "cuda:0", gemm=a.mode)
        data = E.CachedEpoch(tmp, a.batch, 1, augment=True, seed=0)
        warm = make_train_batch(503, a.batch, a.size, a.size)
        w = {k: torch.from_numpy(v).cuda() for k, v in warm.items()}
        for _ in range(2):                                            # allocator, workspaces, code objects
            tr.step(w["lr"], w["hr"], {k: w["out_" + k] for k in E.EXPERTS}, {k: w["feat_" + k] for k in E.EXPERTS})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = E.train_epoch(tr, data, 0, a.accum)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        n = res["micro_batches"] * a.batch
        print(json.dumps({"samples": n, "size": a.size, "batch": a.batch, "accum": a.accum, "mode": a.mode, "epoch_s": wall,
                          "samples_per_s": n / wall, "ms_per_micro_batch": 1e3 * wall / max(1, res["micro_batches"]),
                          "data_wait_s": data.wait_s, "data_wait_share": data.wait_s / wall, "optimizer_steps": res["optimizer_steps"],
                          "loss": res["loss"], "cache_write_s": t_write}), flush=True)


if __name__ == "__main__":
    main()
