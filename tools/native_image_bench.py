"""ff_forward_image_u8 on a DIV2K-validation-sized image: ms per 510x339 uint8 image through a 128/32 tile plan at B = 1, 2 and 4 tiles
per replay (eager launches from C, and the call captured in a HIP graph), beside the plugin's _tiled_forward(model, lr, 128, 32) with
its uint8 conversions on the same box; the variants alternate round by round.  Every native result is compared with the plugin's bytes.
Writes profiles/native_image.json.  python tools/native_image_bench.py [--rounds 5] [--mode bf16x3]

--ensemble: the same protocol for the x8 self-ensemble -- ff_forward_image_ens_u8 at B = 1, 2, 4 beside the plugin's ensemble forced onto
tiles (model.self_ensemble with _tiled_forward and its two graph lanes as `run`) -- and, on a 2040x1356 canvas, ff_tile_fold_d4 for an
even-k and an odd-k code beside the two launches it replaces (ff_tile_normalize + ff_d4_rect_nchw).  Writes profiles/native_image_ens.json."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import models.team29_FreqFusion.io as plug  # noqa: E402
from isr2_amd import ops, plan  # noqa: E402
from isr2_amd.model import FreqFusionHIP  # noqa: E402
from isr2_amd.weights import synth_state_dict  # noqa: E402

H, W, TILE, OVERLAP = 339, 510, 128, 32


def fold_bench(dev, iters=50):
    """ff_tile_fold_d4 against ff_tile_normalize + ff_d4_rect_nchw on the HR canvas of the 510x339 image, accumulating (the case seven of
    eight variants take): device events around `iters` back-to-back launches, the two forms alternating round by round.  GB/s counts
    the bytes each form has to move per pixel: 16 read + 12 read + 12 written = 40 fused, 28 + 36 = 64 in two launches."""
    Hc, Wc = 4 * H, 4 * W
    P = Hc * Wc
    rng = np.random.default_rng(3)
    acc = torch.from_numpy(rng.random((1, 3, Hc, Wc), dtype=np.float32)).to(dev)
    wsum = torch.from_numpy(rng.choice(np.array([0.25, 1.0, 2.0], dtype=np.float32), size=(1, 1, Hc, Wc))).to(dev)
    tmp = torch.empty_like(acc)
    res = {"canvas": [Hc, Wc], "iters": iters, "bytes_per_pixel": {"fused": 40, "two_launches": 64},
           "what": "device events around back-to-back launches with accum = 1, scale = 1; median of 5 alternating rounds; the two-launch "
                   "form normalises a canvas in place (its copy is not counted) and then folds it"}
    for name, code in (("even_k_code3", 3), ("odd_k_code5", 5)):
        ens = torch.zeros((1, 3, Wc, Hc) if code & 4 else (1, 3, Hc, Wc), device=dev)
        ref = torch.zeros_like(ens)
        ops.tile_fold_d4(acc, wsum, code, ens=ens, accum=True)
        tmp.copy_(acc)
        ops.tile_normalize(tmp, wsum)
        ops.d4_rect(tmp, code, out=ref, accum=True)
        same = bool(torch.equal(ens, ref))

        def fused():
            ops.tile_fold_d4(acc, wsum, code, ens=ens, accum=True)

        def pair():
            ops.tile_normalize(tmp, wsum)
            ops.d4_rect(tmp, code, out=ref, accum=True)

        us = {"fused": [], "two_launches": []}
        for _ in range(5):
            for k, fn in (("fused", fused), ("two_launches", pair)):
                fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / iters)
        res[name] = {"bits_equal": same}
        for k, v in us.items():
            t = float(np.median(v))
            res[name][k] = {"us": t, "GB_per_s": res["bytes_per_pixel"][k] * P / t / 1e3}
            print(f"fold {name:14s} {k:13s} {t:8.1f} us  {res[name][k]['GB_per_s']:7.0f} GB/s   bits equal: {same}", flush=True)
    return res


def ensemble_main(a):
    """--ensemble: the protocol of main() for ff_forward_image_ens_u8 (eager launches from C; codes = ops.D4_ENSEMBLE)."""
    dev = torch.device("cuda:0")
    ops.set_gemm_mode(a.mode)
    model = FreqFusionHIP(synth_state_dict(1234), dev)
    img = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    codes = tuple(ops.D4_ENSEMBLE)

    def plugin():
        lr = ops.u8_to_f32_image(img)
        return ops.f32_to_u8_image(model.self_ensemble(lr, codes=codes, run=lambda v: plug._tiled_forward(model, v, TILE, OVERLAP, 4, dev)))

    want = plugin().clone()
    ny, nx = len(plug._tile_positions(H, TILE, TILE - OVERLAP)), len(plug._tile_positions(W, TILE, TILE - OVERLAP))
    variants, nats, equal = {"plugin_ensemble_tiled": plugin}, [], {}
    with tempfile.TemporaryDirectory() as d:
        for B in [int(b) for b in a.batches.split(",")]:
            stem = os.path.join(d, f"t{TILE}b{B}")
            tiles = torch.from_numpy(np.random.default_rng(B).random((B, 3, TILE, TILE), dtype=np.float32)).to(dev)
            info = plan.export_plan(model, tiles, stem)
            nat = plan.NativeModel(stem + ".ffplan", stem + ".ffwts")
            nats.append(nat)
            work = torch.empty(nat.image_ens_workspace_bytes(H, W), device=dev, dtype=torch.uint8)
            got = nat.forward_image_ens_u8(img, OVERLAP, codes, work)         # also the warm-up of this variant
            torch.cuda.synchronize()
            equal[f"B{B}"] = bool(torch.equal(got, want))
            print(f"B = {B}: plan of {info['calls']} launches, work {work.numel() / 1e6:.1f} MB, bytes equal to the plugin's ensemble: {equal[f'B{B}']}", flush=True)
            variants[f"native_ens_eager_B{B}"] = (lambda n=nat, w=work: n.forward_image_ens_u8(img, OVERLAP, codes, w))
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):                                      # alternating: one image per variant per round
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
        print("round done", flush=True)
    res = {"image": [H, W], "tile": TILE, "overlap": OVERLAP, "tiles_per_variant": ny * nx, "codes": list(codes), "mode": a.mode, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0),
           "what": "host wall time around one image (all variants of the ensemble), ending in a device synchronise; uint8 in, uint8 out, no PNG I/O; "
                   "synthetic weights; the native call is not captured in a graph here: unmeasured",
           "bytes_equal_to_plugin": equal,
           "ms_per_image": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()},
           "fold": fold_bench(dev)}
    for k, v in res["ms_per_image"].items():
        print(f"{k:24s} median {v['median']:8.2f} ms   (min {v['min']:.2f}, max {v['max']:.2f})")
    out = a.out if a.out else os.path.join(ROOT, "profiles", "native_image_ens.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for nat in nats:
        nat.close()
    ok = all(equal.values()) and all(res["fold"][k]["bits_equal"] for k in ("even_k_code3", "odd_k_code5"))
    if not ok:
        raise SystemExit(f"native_image_bench: a native result differs from the plugin's: {equal}, fold {res['fold']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensemble", action="store_true", help="time ff_forward_image_ens_u8 and ff_tile_fold_d4 instead (profiles/native_image_ens.json)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mode", default="bf16x3", choices=["bf16x3", "bf16"])
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--out", default=None, help="default: profiles/native_image.json, with --ensemble profiles/native_image_ens.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("native_image_bench: needs the GPU (a timing taken elsewhere says nothing)")
    if a.ensemble:
        return ensemble_main(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "native_image.json")
    dev = torch.device("cuda:0")
    ops.set_gemm_mode(a.mode)
    model = FreqFusionHIP(synth_state_dict(1234), dev)
    img = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)

    def plugin():
        return ops.f32_to_u8_image(plug._tiled_forward(model, ops.u8_to_f32_image(img), TILE, OVERLAP, 4, dev))

    want = plugin().clone()
    ny, nx = len(plug._tile_positions(H, TILE, TILE - OVERLAP)), len(plug._tile_positions(W, TILE, TILE - OVERLAP))
    variants, nats, keep, equal = {"plugin_tiled_forward": plugin}, [], [], {}
    with tempfile.TemporaryDirectory() as d:
        for B in [int(b) for b in a.batches.split(",")]:
            stem = os.path.join(d, f"t{TILE}b{B}")
            tiles = torch.from_numpy(np.random.default_rng(B).random((B, 3, TILE, TILE), dtype=np.float32)).to(dev)
            info = plan.export_plan(model, tiles, stem)
            nat = plan.NativeModel(stem + ".ffplan", stem + ".ffwts")
            nats.append(nat)
            work = torch.empty(nat.image_workspace_bytes(H, W), device=dev, dtype=torch.uint8)
            got = nat.forward_image_u8(img, OVERLAP, work)
            torch.cuda.synchronize()
            equal[f"B{B}"] = bool(torch.equal(got, want))
            print(f"B = {B}: plan of {info['calls']} launches, work {work.numel() / 1e6:.1f} MB, bytes equal to the plugin's: {equal[f'B{B}']}", flush=True)
            variants[f"native_eager_B{B}"] = (lambda n=nat, w=work: n.forward_image_u8(img, OVERLAP, w))
            out = torch.empty_like(got)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                rc = nat.L.ff_forward_image_u8(nat.h, img.data_ptr(), H, W, OVERLAP, out.data_ptr(), work.data_ptr(), work.numel(),
                                               torch.cuda.current_stream().cuda_stream)
            assert rc == 0, nat.L.ff_last_error()
            g.replay()
            torch.cuda.synchronize()
            equal[f"B{B}_graph"] = bool(torch.equal(out, want))
            keep.append((g, out, work))
            variants[f"native_graph_B{B}"] = g.replay
    for fn in variants.values():                                   # every shape the timed window uses is warm
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):                                      # alternating: one image per variant per round
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {"image": [H, W], "tile": TILE, "overlap": OVERLAP, "tiles": ny * nx, "mode": a.mode, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "what": "host wall time around one image, ending in a device synchronise; uint8 in, uint8 out, no PNG I/O; synthetic weights",
           "bytes_equal_to_plugin": equal,
           "ms_per_image": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()}}
    for k, v in res["ms_per_image"].items():
        print(f"{k:24s} median {v['median']:8.2f} ms   (min {v['min']:.2f}, max {v['max']:.2f})")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for nat in nats:
        nat.close()
    if not all(equal.values()):
        raise SystemExit(f"native_image_bench: a native result differs from the plugin's: {equal}")


if __name__ == "__main__":
    main()
