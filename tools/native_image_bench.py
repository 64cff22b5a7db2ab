"""ff_forward_image_u8 on a DIV2K-validation-sized image: ms per 510x339 uint8 image through a 128/32 tile plan at B = 1, 2 and 4 tiles
per replay (eager launches from C, and the call captured in a HIP graph), beside the plugin's _tiled_forward(model, lr, 128, 32) with
its uint8 conversions on the same box; the variants alternate round by round.  Every native result is compared with the plugin's bytes.
Writes profiles/native_image.json.  python tools/native_image_bench.py [--rounds 5] [--mode bf16x3]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mode", default="bf16x3", choices=["bf16x3", "bf16"])
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_image.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("native_image_bench: needs the GPU (a timing taken elsewhere says nothing)")
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
