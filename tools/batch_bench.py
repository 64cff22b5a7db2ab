"""Batched HAT, DAT, NAFNet and fusion stack against the sequential loop over the same images, on one MI355X, in one process:
    python tools/batch_bench.py [--cases 64x64x5,64x64x16,256x256x2] [--modes bf16,bf16x3] [--reps 5] [--rounds 5] [--json PATH]
hat:     HatHIP.forward(lr [B,3,h,w]) (one launch per op for the batch) and the loop `for b: HatHIP.forward(lr[b:b+1])`, each captured
         into one HIP graph and replayed between device events, alternating over --rounds rounds; medians and min..max per form.  The
         outputs of the two graphs are compared bit for bit.  `gain_exceeds_loop_spread` says whether the loop's median minus the
         batch's median is larger than the loop's own min..max spread over the rounds, i.e. whether the gap is more than noise
         (`loss_exceeds_loop_spread`: the same for a batch that is SLOWER than the loop).
nafnet:  the same two forms of NafnetHIP.forward, the same protocol.
dat:     the same two forms of DatHIP.forward, the same protocol.
fusion:  the same two forms of FusionHIP.forward(lr, experts) on given (random) expert outputs [B,3,4h,4w]: no expert runs.
forward: the whole FreqFusionHIP.forward(lr [B,3,h,w]) against the form it had while the fusion stack was per image: the three experts
         batched on their three streams, FusionHIP.pre image by image behind NAFNet, then FusionHIP.forward image by image.
streams: what each of the three streams of model.experts_with_features carries for one group of --group patches of 64x64 (the cache
         builder's unit): HAT, DAT and NAFNet batched and patch by patch, each graph-replayed alone -- the longest bounds the group.
One JSON line per section; --json also writes them to a file."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def _capture(fn):
    """fn() warmed up on a side stream, then captured: -> (graph, what fn returned during the capture)."""
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        fn()
    cur.wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    g.replay()
    torch.cuda.synchronize()
    return g, out


def _timed(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "rounds": [round(t, 4) for t in v]}


def _alternate(graphs, reps, rounds):
    ms = {k: [] for k in graphs}
    for _ in range(rounds):                                        # alternate: clocks and the host are shared by the forms
        for k, g in graphs.items():
            ms[k].append(_timed(g, reps))
    return ms


def expert_section(a, hat, ops, name):
    """`hat` is the expert (HatHIP, DatHIP or NafnetHIP).  NAFNet's zero-padded input belongs to the graphs that are captured here."""
    res = []
    key = (id(hat), "batch_bench", name)
    ops.set_capture_key(key)
    try:
        _expert_cases(a, hat, ops, res)
    finally:
        ops.set_capture_key(None)
        torch.cuda.synchronize()
        ops.drop_persistent(key=key)
    return {"section": name, "reps": a.reps, "rounds": a.rounds, "cases": res}


def _expert_cases(a, hat, ops, res, batched=None, loop_of=None):
    """batched(lr) / loop_of(lr, o_loop)() default to the expert's forward on the batch / image by image into o_loop."""
    for mode in a.modes.split(","):
        ops.set_gemm_mode(mode)
        for case in a.cases.split(","):
            h, w, B = (int(v) for v in case.split("x"))
            lr = torch.rand((B, 3, h, w), device="cuda", generator=torch.Generator(device="cuda").manual_seed(h + B))
            o_loop = torch.empty((B, 3, 4 * h, 4 * w), device="cuda")

            def loop():
                for b in range(B):
                    hat.forward(lr[b:b + 1], out=o_loop[b:b + 1])
                return o_loop

            g_b, o_b = _capture((lambda: batched(lr)) if batched is not None else (lambda: hat.forward(lr)))
            g_l, _ = _capture(loop_of(lr, o_loop) if loop_of is not None else loop)
            same = bool(torch.equal(o_b, o_loop))
            ms = _alternate({"batched": g_b, "loop": g_l}, a.reps, a.rounds)
            sb, sl = _stats(ms["batched"]), _stats(ms["loop"])
            res.append({"mode": mode, "lr": [h, w], "B": B, "tokens": B * ((h + 15) // 16 * 16) * ((w + 15) // 16 * 16),
                        "loss_exceeds_loop_spread": bool(sb["median"] - sl["median"] > sl["max"] - sl["min"]),
                        "ms_batched": sb, "ms_loop": sl, "loop_over_batched": round(sl["median"] / sb["median"], 4),
                        "ms_per_image_batched": round(sb["median"] / B, 4), "ms_per_image_loop": round(sl["median"] / B, 4),
                        "gain_exceeds_loop_spread": bool(sl["median"] - sb["median"] > sl["max"] - sl["min"]), "bit_identical": same})
            del g_b, g_l
            torch.cuda.synchronize()


def fusion_section(a, model, ops):
    """FusionHIP.forward on given expert outputs: one call for the batch against one call per image."""
    fus, res, ex = model.fusion, [], {}
    key = (id(fus), "batch_bench", "fusion")

    def experts(lr):                                               # made once per case (the first, un-captured warm-up call)
        B, _, h, w = lr.shape
        if ex.get("for") is not lr:
            g = torch.Generator(device="cuda").manual_seed(h + 7 * B)
            ex.update({k: torch.rand((B, 3, 4 * h, 4 * w), device="cuda", generator=g) for k in ("hat", "dat", "nafnet")})
            ex["for"] = lr
        return {k: ex[k] for k in ("hat", "dat", "nafnet")}

    def loop_of(lr, o_loop):
        def loop():
            e = experts(lr)
            for b in range(lr.shape[0]):
                fus.forward(lr[b:b + 1], {k: v[b:b + 1] for k, v in e.items()}, out=o_loop[b:b + 1])
            return o_loop
        return loop

    ops.set_capture_key(key)                                       # the concat buffers belong to the graphs captured here
    try:
        _expert_cases(a, fus, ops, res, batched=lambda lr: fus.forward(lr, experts(lr)), loop_of=loop_of)
    finally:
        ops.set_capture_key(None)
        torch.cuda.synchronize()
        ops.drop_persistent(key=key)
    return {"section": "fusion", "reps": a.reps, "rounds": a.rounds, "cases": res}


def forward_section(a, model, ops):
    """FreqFusionHIP.forward on a batch against the form with the per-image fusion stack (experts batched on three streams)."""
    res = []
    key = (id(model), "batch_bench", "forward")
    fus = model.fusion

    def loop_of(lr, o_loop):
        def loop():
            B = lr.shape[0]
            with model._fork(mark=False) as (s1, s2, made):
                with torch.cuda.stream(s1):
                    dat = model.dat.forward(lr)
                with torch.cuda.stream(s2):
                    naf = model.nafnet.forward(lr)
                    pres = [fus.pre(lr[b:b + 1]) for b in range(B)]
                hat = model.hat.forward(lr)
                made += (dat, naf, *(t for p in pres for t in p.values()))
            for b in range(B):
                fus.forward(lr[b:b + 1], {"hat": hat[b:b + 1], "dat": dat[b:b + 1], "nafnet": naf[b:b + 1]}, pre=pres[b], out=o_loop[b:b + 1])
            return o_loop
        return loop

    ops.set_capture_key(key)
    try:
        _expert_cases(a, model, ops, res, batched=lambda lr: model.forward(lr), loop_of=loop_of)
    finally:
        ops.set_capture_key(None)
        torch.cuda.synchronize()
        ops.drop_persistent(key=key)
    return {"section": "forward", "reps": a.reps, "rounds": a.rounds, "multi_stream": bool(model.multi_stream), "cases": res}


def streams_section(a, model, ops):
    ops.set_gemm_mode(a.streams_mode)
    B, p = a.group, 64
    lr = torch.rand((B, 3, p, p), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))

    def per_patch(net):
        def run():
            return [net.forward(lr[b:b + 1], feats={}) for b in range(B)]
        return run

    key = (id(model), "batch_bench")
    ops.set_capture_key(key)                                       # NAFNet's zero-padded input belongs to the captured graphs
    try:
        graphs = {"hat_batched": _capture(lambda: model.hat.forward(lr, feats={}))[0],
                  "hat_per_patch": _capture(per_patch(model.hat))[0],
                  "dat_batched": _capture(lambda: model.dat.forward(lr, feats={}))[0],
                  "dat_per_patch": _capture(per_patch(model.dat))[0],
                  "nafnet_batched": _capture(lambda: model.nafnet.forward(lr, feats={}))[0],
                  "nafnet_per_patch": _capture(per_patch(model.nafnet))[0]}
    finally:
        ops.set_capture_key(None)
    ms = _alternate(graphs, a.reps, a.rounds)
    st = {k: _stats(v) for k, v in ms.items()}
    now = {k: st[k]["median"] for k in ("hat_batched", "dat_per_patch", "nafnet_batched")}
    allb = {k: st[k]["median"] for k in ("hat_batched", "dat_batched", "nafnet_batched")}
    after = {k: st[k]["median"] for k in ("hat_batched", "dat_per_patch", "nafnet_per_patch")}
    before = {k: st[k]["median"] for k in ("hat_per_patch", "dat_per_patch", "nafnet_per_patch")}
    out = {"section": "streams", "mode": a.streams_mode, "group": B, "patch": p, "ms_per_group": st,
           "longest_stream_per_patch_hat": max(before, key=before.get), "longest_stream_batched_hat": max(after, key=after.get),
           "longest_stream_batched_hat_nafnet": max(now, key=now.get), "longest_stream_all_batched": max(allb, key=allb.get)}
    graphs.clear()
    torch.cuda.synchronize()
    ops.drop_persistent(key=key)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64x64x5,64x64x16,256x256x2", help="comma separated h x w x B")
    ap.add_argument("--modes", default="bf16,bf16x3")
    ap.add_argument("--reps", type=int, default=5, help="graph replays per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds; medians and min..max are reported")
    ap.add_argument("--group", type=int, default=5, help="streams section: patches per group")
    ap.add_argument("--streams-mode", default="bf16x3")
    ap.add_argument("--section", default="all", choices=("all", "hat", "nafnet", "dat", "fusion", "forward", "streams"))
    ap.add_argument("--json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_bench: needs an MI355X (no CPU path)")
    from isr2_amd import ops
    from isr2_amd.model import FreqFusionHIP
    from isr2_amd.weights import synth_state_dict
    model = FreqFusionHIP(synth_state_dict(1234), "cuda:0")
    out = []
    with torch.no_grad():
        if a.section in ("all", "hat"):
            out.append(expert_section(a, model.hat, ops, "hat"))
            print(json.dumps(out[-1]), flush=True)
        if a.section in ("all", "nafnet"):
            out.append(expert_section(a, model.nafnet, ops, "nafnet"))
            print(json.dumps(out[-1]), flush=True)
        if a.section in ("all", "dat"):
            out.append(expert_section(a, model.dat, ops, "dat"))
            print(json.dumps(out[-1]), flush=True)
        if a.section in ("all", "fusion"):
            out.append(fusion_section(a, model, ops))
            print(json.dumps(out[-1]), flush=True)
        if a.section in ("all", "forward"):
            out.append(forward_section(a, model, ops))
            print(json.dumps(out[-1]), flush=True)
        if a.section in ("all", "streams"):
            out.append(streams_section(a, model, ops))
            print(json.dumps(out[-1]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
