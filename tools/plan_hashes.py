"""Fingerprints of the recorded launch plans, for host refactors that must not change a launch.

    python tools/plan_hashes.py --mode bf16 [--out FILE]

builds FreqFusionHIP(synth_state_dict(1234)), records plan.export_plan(..., verify=True) for every case of the mode into a temporary
directory and prints ONE JSON object: case -> {sha256 of the .ffplan, calls, streams, workspace_bytes}.  The .ffplan holds every
launch with its arguments and stream, the weight slot names and the packed workspace offsets, so equal hashes on two trees (same
kernel library, same GPU) mean the host issues the same work.  One process per mode: run it on both trees and compare.

Cases (key "mode/B x LR size/schedule"): B == 1 on bench.make_tile(100, size) for size 64 and 256; B == 2 on tiles 100 and 101 of size
32 (not in f32 mode, where the batch runs HAT per image anyway).  Each on three streams ("multi") and on one ("single").
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from isr2_amd import ops, plan  # noqa: E402
from isr2_amd.model import FreqFusionHIP  # noqa: E402
from isr2_amd.weights import synth_state_dict  # noqa: E402


def inputs(mode: str):
    yield "1x64", bench.make_tile(100, 64)
    yield "1x256", bench.make_tile(100, 256)
    if mode != "f32":
        yield "2x32", torch.cat([bench.make_tile(100, 32), bench.make_tile(101, 32)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=("bf16", "bf16x3", "f32"))
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    args = ap.parse_args()
    ops.set_gemm_mode(args.mode)
    model = FreqFusionHIP(synth_state_dict(1234), "cuda:0")
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for shape, lr in inputs(args.mode):
            for sched, multi in (("multi", True), ("single", False)):
                stem = os.path.join(tmp, f"{shape}_{sched}")
                info = plan.export_plan(model, lr.cuda(), stem, multi_stream=multi, verify=True)
                with open(stem + ".ffplan", "rb") as f:
                    sha = hashlib.sha256(f.read()).hexdigest()
                res[f"{args.mode}/{shape}/{sched}"] = {"sha256": sha, "calls": info["calls"], "streams": info["streams"],
                                                       "workspace_bytes": info["workspace_bytes"]}
                os.remove(stem + ".ffplan")
                os.remove(stem + ".ffwts")
    txt = json.dumps(res)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
