"""Time live-expert training epochs on one MI355X, next to the cached epoch of tools/epoch_bench.py measured in the same session.

    python tools/live_bench.py [--images 48] [--lr-size 128] [--batch 14] [--repeat 7] [--accum 2] [--rounds 3] [--mode f32]
                               [--expert-mode bf16x3] [--cached-samples 112] [--color-jitter] [--out FILE]

A seeded synthetic folder of PNG pairs is written to a temporary directory and decoded into an isr2_amd.epoch.ImagePool.  Then:
  * parts of one micro-batch, device events over repeated calls after a warm-up: the sampler launch (ops.sample_pairs_u8 -- with the
    bytes it moves: 3 B p^2 17 read as uint8, 4x that written as fp32 -> GB/s), the expert graph replay, the training step
    (forward_backward + optimizer_step on a fixed micro-batch);
  * whole epochs through epoch.train_epoch, a host clock around work that ends in a device synchronise: LiveEpoch(overlap=False) and
    LiveEpoch(overlap=True) ALTERNATING for --rounds rounds in this one process.  Per form: samples/s of every round, their median and
    spread (max - min); the overlap's margin over the single lane is compared with five times the single lane's own spread;
  * the cached epoch: tools/epoch_bench.py as a child process after the live runs (the cached loader is the code path of the parent
    commit), --cached-samples synthetic samples.
  * --color-jitter: both live forms are LiveEpoch(color_jitter=True) -- the reference's defaults, about half of the samples applied --,
    and the two launches of ops.color_jitter_pairs (csrc/color_jitter.hip) on a sampled micro-batch are reported per micro-batch beside
    sampler, experts and step: once with the epoch's table as drawn and once with every sample applied.  To compare with the plain
    loop, run the tool with and without the flag in one job, alternating the two (one process each: a process keeps the two forms and
    the streams it always had).
One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def write_folder(root, n, lr_size, seed=4242):
    """n seeded PNG pairs: LR lr_size^2 of blocky noise, HR its nearest x4 with detail noise (every image decodes to fresh bytes)."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    hr_dir, lr_dir = os.path.join(root, "hr"), os.path.join(root, "lr")
    os.makedirs(hr_dir)
    os.makedirs(lr_dir)
    for i in range(n):
        base = rng.integers(0, 256, (lr_size // 4, lr_size // 4, 3), dtype=np.uint8)
        lr = np.repeat(np.repeat(base, 4, axis=0), 4, axis=1) ^ rng.integers(0, 16, (lr_size, lr_size, 3), dtype=np.uint8)
        hr = np.repeat(np.repeat(lr, 4, axis=0), 4, axis=1) ^ rng.integers(0, 8, (4 * lr_size, 4 * lr_size, 3), dtype=np.uint8)
        Image.fromarray(lr).save(os.path.join(lr_dir, f"im{i:04d}.png"), compress_level=1)
        Image.fromarray(hr).save(os.path.join(hr_dir, f"im{i:04d}.png"), compress_level=1)
    return hr_dir, lr_dir


def event_ms(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--batch", type=int, default=14)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--accum", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mode", default="f32")
    ap.add_argument("--expert-mode", default="bf16x3")
    ap.add_argument("--cached-samples", type=int, default=112)
    ap.add_argument("--color-jitter", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("live_bench: no GPU -- nothing here can be measured without one")
    from isr2_amd import epoch as E
    from isr2_amd import ops
    from isr2_amd.model import FreqFusionHIP
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    res = {"config": vars(a).copy(), "device": torch.cuda.get_device_name(0)}
    ops.set_gemm_mode(a.expert_mode)
    B, p = a.batch, a.patch
    with tempfile.TemporaryDirectory() as tmp:
        hr_dir, lr_dir = write_folder(tmp, a.images, a.lr_size)
        model = FreqFusionHIP(synth_state_dict(1234), "cuda:0")
        tr = FusionTrainer(synth_state_dict(1234, parts=("fusion", "collab")), "cuda:0", gemm=a.mode)
        t0 = time.perf_counter()
        pool = E.ImagePool(hr_dir, lr_dir, patch=p, readers=8)
        t_pool = time.perf_counter() - t0
        res["pool"] = {"images": len(pool), "bytes": pool.total_bytes, "build_s": t_pool, "images_per_s": len(pool) / t_pool}
        names = {False: "overlap_off", True: "overlap_on"}
        jitter = True if a.color_jitter else None
        forms = {False: E.LiveEpoch(model, pool, B, a.repeat, augment=True, seed=0, overlap=False, color_jitter=jitter),
                 True: E.LiveEpoch(model, pool, B, a.repeat, augment=True, seed=0, overlap=True, color_jitter=jitter)}
        try:
            single = forms[False]
            L = single._lanes[0]
            desc = single.descriptors(0)
            desc_dev = torch.from_numpy(desc).cuda()
            k = [0]

            def sample():
                b = k[0] % desc.shape[0]
                k[0] += 1
                ops.sample_pairs_u8(pool.buf, desc[b], p, desc_dev=desc_dev[b], out=(L["lr"], L["hr"]))

            def step():
                tr.forward_backward(L["lr"], L["hr"], L["outs"], L["feats"])
                tr.optimizer_step()

            L["graph"].replay()                                       # expert outputs of a real micro-batch for the step's timing
            for _ in range(2):
                step()
            moved = 3 * B * p * p * 17 * (1 + 4)                      # uint8 read + fp32 written, LR + HR
            ms_sample = event_ms(sample, 50)
            res["parts_ms_per_micro_batch"] = {"sampler_launch": ms_sample, "sampler_bytes": moved, "sampler_GBps": moved / ms_sample / 1e6,
                                               "expert_replay": event_ms(L["graph"].replay, 10), "step": event_ms(step, 10)}
            if a.color_jitter:
                jit = single.jitter_table(0)
                every = jit.copy()
                every[..., 0] = 1.0

                def jitter_ms(table):
                    dev = torch.from_numpy(table).cuda()

                    def run():                                        # a fresh sample first: the jitter always sees u8 / 255
                        b = k[0] % desc.shape[0]
                        sample()
                        ops.color_jitter_pairs(L["lr"], L["hr"], table[b], table_dev=dev[b])
                    return event_ms(run, 50) - ms_sample

                full = 3 * B * p * p * 17 * 4 * 3                     # fp32 read for the sums, read and written by the pixel pass
                ms_drawn, ms_every = jitter_ms(jit), jitter_ms(every)
                res["parts_ms_per_micro_batch"].update({"jitter_two_launches_as_drawn": ms_drawn, "jitter_applied_share": float(jit[..., 0].mean()),
                                                        "jitter_two_launches_every_sample": ms_every, "jitter_bytes_every_sample": full,
                                                        "jitter_GBps_every_sample": full / ms_every / 1e6,
                                                        "jitter_note": "sampler + jitter timed together, the sampler's own time subtracted"})
            # whole epochs, the forms alternating
            rows = {form: [] for form in forms}
            for form in forms:                                        # one unmeasured epoch each: allocator, second lane's first replay
                E.train_epoch(tr, forms[form], 0, a.accum)
            torch.cuda.synchronize()
            for r in range(a.rounds):
                for form in forms:
                    t0 = time.perf_counter()
                    out = E.train_epoch(tr, forms[form], 1 + r, a.accum)
                    torch.cuda.synchronize()
                    wall = time.perf_counter() - t0
                    n = out["micro_batches"] * B
                    rows[form].append({"round": r, "epoch_s": wall, "samples": n, "samples_per_s": n / wall,
                                       "ms_per_micro_batch": 1e3 * wall / out["micro_batches"], "data_wait_share": forms[form].wait_s / wall,
                                       "loss": out["loss"]})
            summ = {}
            for form, name in names.items():
                v = [x["samples_per_s"] for x in rows[form]]
                summ[name] = {"samples_per_s_median": statistics.median(v), "samples_per_s_min": min(v), "samples_per_s_max": max(v),
                              "samples_per_s_spread": max(v) - min(v), "rounds": rows[form]}
            margin = summ["overlap_on"]["samples_per_s_median"] - summ["overlap_off"]["samples_per_s_median"]
            need = 5 * summ["overlap_off"]["samples_per_s_spread"]
            summ["overlap_margin_samples_per_s"] = margin
            summ["five_times_single_lane_spread"] = need
            summ["overlap_beats_single_lane_by_the_rule"] = bool(margin >= need and margin > 0)
            res["live_epoch"] = summ
        finally:
            for f in forms.values():
                f.close()
    del model, tr, pool
    torch.cuda.empty_cache()
    if a.cached_samples > 0:
        cmd = [sys.executable, os.path.join(ROOT, "tools", "epoch_bench.py"), "--samples", str(a.cached_samples), "--size", str(p), "--batch", str(B),
               "--accum", str(a.accum), "--mode", a.mode]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        res["cached_epoch"] = json.loads(lines[-1]) if r.returncode == 0 and lines else {"unmeasured": f"epoch_bench.py exited with {r.returncode}: {r.stderr[-400:]}"}
    else:
        res["cached_epoch"] = {"unmeasured": "--cached-samples 0"}
    txt = json.dumps(res, indent=1)
    print(txt, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
