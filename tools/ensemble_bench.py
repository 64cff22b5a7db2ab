"""Cost of the x8 geometric self-ensemble on one MI355X, measured in one process:
    python tools/ensemble_bench.py [--dtype bf16] [--reps 10] [--section all|ensemble|kernels]
ensemble: model.self_ensemble(tile, run=model.graphed) against model.graphed(tile) on bench.make_tile(100) (256x256 LR), alternating,
          device events around each; also with the two graph lanes (run_async=model.graphed_async).  Expectation: ratio ~ 8.
kernels:  ff_d4_rect_nchw on [1,3,1024,1024] for one even and one odd code, without and with accum, beside ff_d4_nchw (the training
          loader's kernel, the yardstick) for the same shape and code.  The launches of one variant are captured into one HIP graph
          (a 25 MB permutation takes microseconds: launched from Python one by one, the host would be what is timed) and the graph is
          replayed between device events.  GB/s counts 2 planes of traffic without accum (read src, write dst) and 3 with (+ read dst).
Under `rocprofv3 --kernel-trace --stats -- python tools/ensemble_bench.py --section ensemble` the per-kernel table gives the share of
d4_rect_kernel in the ensemble's kernel time.  One JSON line per section."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def ensemble_section(a):
    import bench
    from isr2_amd import ops
    from isr2_amd.model import FreqFusionHIP
    from isr2_amd.weights import synth_state_dict
    ops.set_gemm_mode(a.dtype)
    model = FreqFusionHIP(synth_state_dict(1234), "cuda:0")
    tile = bench.make_tile(100).cuda()
    out = torch.empty(1, 3, 4 * tile.shape[2], 4 * tile.shape[3], device="cuda")
    one = lambda: model.graphed(tile)                                                          # noqa: E731
    x8 = lambda: model.self_ensemble(tile, run=model.graphed, out=out)                         # noqa: E731
    x8_lanes = lambda: model.self_ensemble(tile, run=model.graphed, run_async=model.graphed_async, out=out)   # noqa: E731
    for f in (one, x8, x8_lanes):                                                              # captures, code objects, allocator
        f()
        f()
    torch.cuda.synchronize()
    ref = x8().clone()
    same = bool(torch.equal(x8_lanes(), ref))
    ms = {"one": [], "x8": [], "x8_lanes": []}
    for _ in range(a.rounds):                                                                  # alternate: the host is shared
        ms["one"].append(_timed(one, 8 * a.reps))
        ms["x8"].append(_timed(x8, a.reps))
        ms["x8_lanes"].append(_timed(x8_lanes, a.reps))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    print(json.dumps({"section": "ensemble", "dtype": a.dtype, "tile": list(tile.shape), "ms_one_pass": med["one"],
                      "ms_ensemble": med["x8"], "ratio": med["x8"] / med["one"], "ms_ensemble_two_lanes": med["x8_lanes"],
                      "ratio_two_lanes": med["x8_lanes"] / med["one"], "lanes_bit_identical": same,
                      "rounds_ms": {k: [round(t, 3) for t in v] for k, v in ms.items()}}), flush=True)


def kernels_section(a):
    from isr2_amd import ops
    shape = (1, 3, 1024, 1024)
    x = torch.randn(shape, device="cuda")
    dst = torch.zeros(shape, device="cuda")
    plane_bytes = 4 * x.numel()
    n = a.launches
    res = {}
    for code in (3, 5):                                                                        # even k (both flips), odd k (one flip + a quarter turn)
        cd = torch.tensor([code], dtype=torch.int32).cuda()
        variants = {"d4_rect": (lambda: ops.d4_rect(x, code, out=dst), 2),
                    "d4_rect_accum": (lambda: ops.d4_rect(x, code, out=dst, accum=True, scale=0.125), 3),
                    "d4_nchw": (lambda: ops.d4_nchw(x, [code], out=dst, codes_dev=cd), 2)}
        graphs = {}
        for name, (fn, _) in variants.items():
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(n):
                    fn()
            g.replay()
            graphs[name] = g
        torch.cuda.synchronize()
        us = {k: [] for k in variants}
        for _ in range(a.rounds):
            for name, g in graphs.items():
                us[name].append(1e3 * _timed(g.replay, 5) / n)
        for name, (_, planes) in variants.items():
            t = sorted(us[name])[len(us[name]) // 2]
            res[f"{name}_code{code}"] = {"us": round(t, 3), "GBps": round(planes * plane_bytes / t / 1e3, 1)}
        res[f"rect_over_nchw_code{code}"] = round(res[f"d4_nchw_code{code}"]["us"] / res[f"d4_rect_code{code}"]["us"], 3)
    print(json.dumps({"section": "kernels", "shape": list(shape), "launches_per_graph": n, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--reps", type=int, default=5, help="ensembles per timed window (8x as many single passes)")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds; the median is reported")
    ap.add_argument("--launches", type=int, default=100, help="permutation launches per captured graph")
    ap.add_argument("--section", default="all", choices=("all", "ensemble", "kernels"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench: needs an MI355X (no CPU path)")
    if a.section in ("all", "kernels"):
        kernels_section(a)
    if a.section in ("all", "ensemble"):
        ensemble_section(a)


if __name__ == "__main__":
    main()
