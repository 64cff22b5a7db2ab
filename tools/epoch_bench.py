"""Time one whole training epoch from a cache directory on one MI355X: N synthetic samples (tests/golden/train_inputs.make_train_batch)
are written to a temporary cache, one epoch runs through isr2_amd.epoch (reader thread -> pinned slot -> one upload -> ff_d4_nchw ->
accumulated steps), and samples/s plus the share of wall time the stepping thread waited for data are printed.
    python tools/epoch_bench.py [--samples 256] [--size 64] [--batch 14] [--accum 2] [--mode f32] [--d4-only]
    python tools/epoch_bench.py --resident [--rounds 3] [--readers 8] [--probe-gb 0] [--out profiles/resident_cache.json]
--d4-only: time the eight augmentation launches of one micro-batch alone (under rocprofv3 --kernel-trace --stats the per-kernel
table comes out of the same command) and print the GB/s of the largest tensor.
--resident: the same synthetic cache through epoch.CachedEpoch AND through epoch.ResidentCache / ResidentEpoch in ONE call, alternating
--rounds times (at least 3): samples/s and data-wait share of each epoch, the pool's load time and samples/s at --readers, the step-only
epoch (train_epoch over one fixed device micro-batch: the ceiling of both) and the gather launch alone (device events around 60
back-to-back launches into one reused output buffer, us and GB/s of its 2 x B x sample bytes).  --probe-gb G > 0: allocate G GB beside
the live trainer and the pool and run one accumulation window, to say whether a pool of that size and the step coexist on the device.
The JSON goes to stdout and to --out."""
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
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--readers", type=int, default=8)
    ap.add_argument("--probe-gb", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_cache.json"))
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
                cache.write_sample(tmp, f"s{done + j:05d}", *cache.fields_batch({k: v[j:j + 1] for k, v in d.items()}))
            done += nb
        t_write = time.perf_counter() - t0
        if a.resident:
            return resident(a, tmp, t_write)
        tr = FusionTrainer(synth_state_dict(1234, parts=("fusion", "collab")), "cuda:0", gemm=a.mode)
        data = E.CachedEpoch(tmp, a.batch, 1, augment=True, seed=0)
        warm = make_train_batch(503, a.batch, a.size, a.size)
        w = {k: torch.from_numpy(v).cuda() for k, v in warm.items()}
        for _ in range(2):                                            # allocator, workspaces, code objects
            tr.step(*cache.fields_batch(w))
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


def resident(a, tmp, t_write):
    """--resident: CachedEpoch and ResidentEpoch on the cache in `tmp`, alternating, with the step-only ceiling and the gather alone."""
    import numpy as np
    from train_inputs import make_train_batch
    from isr2_amd import cache, ops
    from isr2_amd import epoch as E
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    rounds = max(3, a.rounds)
    tr = FusionTrainer(synth_state_dict(1234, parts=("fusion", "collab")), "cuda:0", gemm=a.mode)
    w = {k: torch.from_numpy(v).cuda() for k, v in make_train_batch(503, a.batch, a.size, a.size).items()}
    fixed = cache.fields_batch(w)
    for _ in range(2):                                                # allocator, workspaces, code objects
        tr.step(*fixed)
    torch.cuda.synchronize()
    pool = E.ResidentCache(tmp, readers=a.readers)
    cached = E.CachedEpoch(tmp, a.batch, 1, augment=True, seed=0)
    res = E.ResidentEpoch(pool, a.batch, 1, augment=True, seed=0)
    nb = len(res)

    def epoch(data, e):
        if hasattr(data, "wait_s"):
            data.wait_s = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = E.train_epoch(tr, data, e, a.accum)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        n = r["micro_batches"] * a.batch
        wait = getattr(data, "wait_s", 0.0)
        return {"epoch": e, "samples": n, "epoch_s": wall, "samples_per_s": n / wall, "data_wait_s": wait, "data_wait_share": wait / wall, "loss": r["loss"]}

    rows = {"cached_epoch": [], "resident_epoch": [], "step_only": []}
    for e in range(rounds):                                           # alternating, in one process: the three see the same machine
        rows["cached_epoch"].append(epoch(cached, e))
        rows["resident_epoch"].append(epoch(res, e))
        rows["step_only"].append(epoch([fixed] * nb, e))
    # the gather launch alone: every launch draws its own B samples over the whole pool (no launch re-reads the one before it), one
    # reused output buffer
    n_launch, n_warm = 60, 5
    desc = np.stack((np.random.default_rng(0).integers(0, len(pool), size=(n_warm + n_launch, a.batch)),
                     np.broadcast_to(np.arange(a.batch) % 16, (n_warm + n_launch, a.batch))), axis=-1).astype(np.int32)
    desc_dev = torch.from_numpy(desc).cuda()
    flat = torch.empty(res.out_floats, dtype=torch.float32, device="cuda")
    for i in range(n_warm):
        ops.gather_d4_fields(pool.buf, len(pool), res.fields, desc_dev[i], flat, desc_host=desc[i])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n_warm, n_warm + n_launch):
        ops.gather_d4_fields(pool.buf, len(pool), res.fields, desc_dev[i], flat)
    e1.record()
    torch.cuda.synchronize()
    us = 1e3 * e0.elapsed_time(e1) / n_launch
    sample_bytes = 4 * sum(int(np.prod(pool.shapes[k])) for k in E.FIELDS)
    moved = 2 * a.batch * sample_bytes
    med = lambda k, f: float(np.median([r[f] for r in rows[k]]))      # noqa: E731
    out = {"protocol": f"one process, one MI355X: {a.samples} synthetic samples at {a.size}x{a.size} LR written to a temporary cache, trainer warmed "
                       f"by 2 steps, then {rounds} rounds alternating CachedEpoch / ResidentEpoch / step-only epochs of {nb} micro-batches "
                       f"(batch {a.batch}, accumulation {a.accum}, mode {a.mode}, augmentation on); host clock around train_epoch ending in a "
                       "device synchronise; medians over the rounds beside every round",
           "samples": a.samples, "size": a.size, "batch": a.batch, "accum": a.accum, "mode": a.mode, "rounds": rounds, "cache_write_s": t_write,
           "pool": {"bytes": pool.total_bytes, "readers": pool.readers, "load_s": pool.load_s, "load_samples_per_s": len(pool) / pool.load_s,
                    "load_GBps": pool.total_bytes / pool.load_s / 1e9},
           "median": {k: {"samples_per_s": med(k, "samples_per_s"), "data_wait_share": med(k, "data_wait_share")} for k in rows},
           "rounds_detail": rows,
           "gather_alone": {"B": a.batch, "patch": a.size, "launches": n_launch, "us_per_launch": us, "bytes_moved": moved,
                            "GBps": moved / us / 1e3, "sample_bytes": sample_bytes,
                            "note": f"device events around {n_launch} back-to-back launches after {n_warm} warm-up launches, each with its own descriptor; a launch "
                                    f"reads {moved / 2e6:.0f} MB scattered over the {pool.total_bytes / 1e9:.2f} GB pool (larger than the 256 MB Infinity Cache) and "
                                    f"writes {moved / 2e6:.0f} MB into ONE reused buffer (smaller than it): the rate is not an HBM-to-HBM rate"}}
    if a.probe_gb > 0:
        free0, total = torch.cuda.mem_get_info()
        probe = {"GB": a.probe_gb, "device_total_bytes": total, "free_before_bytes": free0, "held_by_torch_before_bytes": torch.cuda.memory_reserved()}
        try:
            big = torch.empty(int(a.probe_gb * 1e9), dtype=torch.uint8, device="cuda")
            torch.cuda.reset_peak_memory_stats()
            r = epoch([fixed] * a.accum, 0)                           # one accumulation window beside the allocation
            probe.update(allocated=True, window_ran=True, window_samples_per_s=r["samples_per_s"], peak_allocated_bytes=torch.cuda.max_memory_allocated(),
                         free_after_bytes=torch.cuda.mem_get_info()[0])
            del big
        except torch.cuda.OutOfMemoryError as e:
            probe.update(allocated=False, error=str(e).splitlines()[0])
        out["coexistence_probe"] = probe
    txt = json.dumps(out, indent=1)
    print(txt, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
