"""Throughput of the cached-expert data-set builder on one MI355X.  A synthetic folder of seeded PNG pairs is written to a temporary
directory; then, alternating in one process, (a) isr2_amd.cache.build_from_folders (with and without the graph replay) and (b) the sequential loop a user would write
around cache.extract (decode, upload, cut the same patches with torch slicing, extract) fill fresh cache directories; (c) is
cache.extract alone over patches already cut on the device (no decoding); (d) with --batch N > 1, build_from_folders(batch=N): the
patches of an image in groups of N, HAT batched.  Also: the GB/s of ff_crop_pairs_u8 and ff_resize_aa at a
2040 x 1356 HR image (DIV2K-sized), and the HR-only mode of the builder.
    python tools/cache_bench.py [--images 12] [--lr-h 128] [--lr-w 160] [--patch 64] [--crops 5] [--rounds 3] [--gemm bf16x3] [--batch 1] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def _kernel_rates(ops):
    h, w, p, n = 339, 510, 64, 50
    g = torch.Generator().manual_seed(0)
    lr_u8 = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).cuda()
    hr_u8 = torch.randint(0, 256, (4 * h, 4 * w, 3), dtype=torch.uint8, generator=g).cuda()
    hr_f = ops.u8_to_f32_image(hr_u8)
    out = {}
    for K in (5, 64):
        pos = [((7 * k) % (h - p + 1), (13 * k) % (w - p + 1)) for k in range(K)]
        run = lambda: ops.crop_pairs_u8(lr_u8, hr_u8, pos, p)                     # noqa: E731 -- includes the K x 2 position upload
        for _ in range(3):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / n
        nbytes = K * 3 * p * p * 17 * 5                                           # uint8 read + fp32 written, LR and HR patches
        out[f"crop_pairs_u8_K{K}_p{p}"] = {"ms_per_call": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6}
    run = lambda: ops.resize_aa(hr_f, (h, w))                                     # noqa: E731
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    nbytes = 4 * 3 * (16 * h * w + h * w)
    out[f"resize_aa_{4 * h}x{4 * w}"] = {"ms_per_call": ms, "bytes": nbytes, "GBps": nbytes / ms / 1e6}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=12)
    ap.add_argument("--lr-h", type=int, default=128)
    ap.add_argument("--lr-w", type=int, default=160)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--crops", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gemm", default="bf16x3")
    ap.add_argument("--batch", type=int, default=1, help="> 1: also time build_from_folders(batch=N)")
    ap.add_argument("--json")
    a = ap.parse_args()
    from PIL import Image
    from isr2_amd import cache, ops
    from isr2_amd.model import FreqFusionHIP
    from isr2_amd.weights import synth_state_dict
    ops.set_gemm_mode(a.gemm)
    model = FreqFusionHIP(synth_state_dict(1234), "cuda:0")
    h, w, p = a.lr_h, a.lr_w, a.patch
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "lr"))
        os.makedirs(os.path.join(tmp, "hr"))
        rng = np.random.default_rng(0)
        for i in range(a.images):
            # smooth seeded content (noise PNGs do not compress: their decode time is not an image's)
            base = rng.random((h // 8 + 2, w // 8 + 2, 3), dtype=np.float32)
            hr = torch.nn.functional.interpolate(torch.from_numpy(base).permute(2, 0, 1)[None], size=(4 * h, 4 * w), mode="bicubic")[0]
            hr = (hr.clamp(0, 1) * 255).round().byte().permute(1, 2, 0).numpy()
            Image.fromarray(hr).save(os.path.join(tmp, "hr", f"img{i:04d}.png"))
            Image.fromarray(np.ascontiguousarray(hr[::4, ::4])).save(os.path.join(tmp, "lr", f"img{i:04d}.png"))
        stems = sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(tmp, "hr")))

        def load(kind, stem):
            return torch.from_numpy(np.asarray(Image.open(os.path.join(tmp, kind, stem + ".png")).convert("RGB"), dtype=np.uint8).copy())

        def cut(index, stem):
            lr, hr = ops.u8_to_f32_image(load("lr", stem).cuda()), ops.u8_to_f32_image(load("hr", stem).cuda())
            for k, (t, l) in enumerate(cache.crop_plan(h, w, p, a.crops, 0, index)):
                yield f"{stem}_p{k}", lr[:, :, t:t + p, l:l + p].contiguous(), hr[0, :, 4 * t:4 * (t + p), 4 * l:4 * (l + p)].contiguous()

        def run_builder(out, **kw):
            res = cache.build_from_folders(model, os.path.join(tmp, "hr"), out, patch=p, crops=a.crops, seed=0, **kw)
            return res["patches_written"], res["seconds"]["total"], res

        def run_loop(out):
            t0 = time.perf_counter()
            n = cache.extract(model, (s for i, stem in enumerate(stems) for s in cut(i, stem)), out)
            torch.cuda.synchronize()
            return n, time.perf_counter() - t0, None

        precut = [s for i, stem in enumerate(stems[:max(1, a.images // 2)]) for s in cut(i, stem)]

        def run_extract_only(out):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = cache.extract(model, precut, out)
            torch.cuda.synchronize()
            return n, time.perf_counter() - t0, None

        variants = {"build_from_folders": lambda o: run_builder(o, lr_dir=os.path.join(tmp, "lr")),
                    "build_from_folders_no_graph": lambda o: run_builder(o, lr_dir=os.path.join(tmp, "lr"), graph=False), "extract_loop": run_loop,
                    "extract_only": run_extract_only, "build_from_folders_hr_only": lambda o: run_builder(o)}
        if a.batch > 1:
            variants[f"build_from_folders_batch{a.batch}"] = lambda o: run_builder(o, lr_dir=os.path.join(tmp, "lr"), batch=a.batch)
        cache.extract(model, precut[:2], os.path.join(tmp, "warm"))                # code objects, allocator, workspaces
        rates = {k: [] for k in variants}
        last = {}
        for r in range(a.rounds):
            for name, fn in variants.items():                                     # alternating: every round runs every variant once
                n, dt, res = fn(os.path.join(tmp, f"{name}_{r}"))
                rates[name].append(n / dt)
                if res is not None:
                    last[name] = res
        kern = _kernel_rates(ops)
    med = {k: statistics.median(v) for k, v in rates.items()}
    secs = last["build_from_folders"]["seconds"]
    out = {"images": a.images, "lr": [h, w], "patch": p, "crops": a.crops, "gemm": a.gemm, "rounds": a.rounds,
           "patches_per_s": {k: {"median": med[k], "runs": v} for k, v in rates.items()},
           "builder_over_extract_loop": med["build_from_folders"] / med["extract_loop"],
           "builder_over_extract_only": med["build_from_folders"] / med["extract_only"],
           "no_graph_builder_over_extract_loop": med["build_from_folders_no_graph"] / med["extract_loop"],
           "builder_stage_seconds": secs, "builder_stage_share_of_wall": {k: v / secs["total"] for k, v in secs.items() if k != "total"},
           "kernels": kern}
    if a.batch > 1:
        name = f"build_from_folders_batch{a.batch}"
        bs = last[name]["seconds"]
        out["batch"] = {"batch": a.batch, "patches_per_s": med[name], "over_batch_1": med[name] / med["build_from_folders"], "stage_seconds": bs,
                        "stage_share_of_wall": {k: v / bs["total"] for k, v in bs.items() if k != "total"}}
    line = json.dumps(out)
    print(line, flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
