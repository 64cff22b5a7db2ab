"""Headline benchmark: output MPix/s of the FreqFusion x4 full 3-expert forward on 256x256 LR tiles.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes its outputs if asked and prints the result line, nothing more.
--full adds, after the timed steps: the per-kernel accounting pass (roofline, stage and kernel breakdowns), the other contraction
modes with their PSNR against the reference's output, the CPU oracle baseline and the training side block (about two minutes).

N > 1: either the driver launches one rank per GPU (torch.distributed.run: RANK / WORLD_SIZE set), or -- when called plainly --
this script starts N fresh child ranks of itself before touching any GPU and relays rank 0's JSON line.

One process per GPU.  A step = one pass of the hot path (HAT-L + DAT + NAFNet-SR + fusion stack) over
one synthetic 256x256 LR tile per GPU (BASELINE.json configs[1]); tiles are independent, so ranks
shard them with NO data-path collective (weak scaling).  The only collective is the one-off RCCL
broadcast of the frozen weights from rank 0.  The steady state is replayed from a HIP graph (the
eager Python launch loop is captured once), inputs are resident in HBM before the timed region.
Rank 0 prints ONE JSON line; see DESIGN.md "Measurement" for how the --full fields (roofline, cpu_baseline, ...) are defined.
--dump-outputs DIR: after the timed steps, the SR output of the last timed step (what a caller of the timed path receives) is
written as DIR/sr.npy, float32 [1, 3, 4*tile, 4*tile] (12 MiB at the default tile; DIR/sr_rank<r>.npy per rank when N > 1).
Above 64 MiB (--tile > 591) the file holds a fixed seeded sample of 16 Mi output values, flattened, in index order.
Weights and tiles are seeded, so two builds run with the same arguments can be compared output for output.
"""
import argparse
import glob
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

TILE = 256
FLOP_PER_TILE = 11295.4e9          # algorithmic 2xMAC FLOPs of one 256x256 LR tile [measured on the reference]
MPIX_PER_TILE = (4 * TILE) ** 2 / 1e6
PEAK_TF = {"f32": 157.3, "bf16": 2500.0, "bf16x2": 2500.0, "bf16x3": 2500.0}   # MI355X_MICROARCH.md dense MFMA peaks
MFMA_PER_ALGO_FLOP = {"f32": 1, "bf16": 1, "bf16x2": 2, "bf16x3": 3}
SEED = 1234
DUMP_MAX_BYTES = 64 * 2 ** 20      # --dump-outputs cap


def make_tile(seed: int, size: int = TILE) -> torch.Tensor:
    """Natural-statistics synthetic LR tile: 1/f-spectrum noise clipped to [0,1]."""
    rng = np.random.default_rng(seed)
    fy = np.fft.fftfreq(size)[:, None]
    fx = np.fft.fftfreq(size)[None, :]
    amp = 1.0 / np.maximum(np.sqrt(fy ** 2 + fx ** 2), 1.0 / size)
    chans = []
    for _ in range(3):
        img = np.real(np.fft.ifft2(amp * np.exp(1j * rng.random((size, size)) * 2 * np.pi)))
        chans.append(np.clip((img - img.mean()) / (img.std() + 1e-8) * 0.2 + 0.5, 0, 1))
    return torch.from_numpy(np.stack(chans)[None].astype(np.float32))


def log(msg: str):
    if int(os.environ.get("RANK", "0")) == 0:
        print(f"[bench +{time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


_T0 = time.perf_counter()


def host_threads() -> int:
    """CPU share of this process (cgroup/affinity aware), capped at 16 -- the GPU box's per-GPU share."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def broadcast_weights(rank: int, world: int, dev):
    """Rank 0 builds the seeded synthetic state dict; everyone else receives it in ONE RCCL broadcast."""
    from isr2_amd.parallel import broadcast_state_dict
    from isr2_amd.weights import param_spec, synth_state_dict
    if world == 1:
        return synth_state_dict(SEED), 0.0
    import torch.distributed as dist
    src = synth_state_dict(SEED) if rank == 0 else None
    torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    sd = broadcast_state_dict(src, param_spec(), rank, world, dev)
    torch.cuda.synchronize()
    return sd, time.perf_counter() - t0


def cpu_model_name() -> str:
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sd, threads: int, tile: int):
    """The CPU oracle (a port of the reference's PyTorch eval path, pinned to it by golden fixtures) timed on this host's
    cores on THE SAME workload as the GPU step: one warm-up on a 64x64 tile (loads the code paths), then one timed
    `tile` x `tile` LR tile (BASELINE.md section 3 / SURVEY 8d)."""
    from oracle import freqfusion_oracle as O
    torch.set_num_threads(threads)
    cpu_sd = {k: v.detach().cpu() for k, v in sd.items()}
    O.forward(cpu_sd, make_tile(3, 64))
    lr = make_tile(100, tile)
    t0 = time.perf_counter()
    O.forward(cpu_sd, lr)
    dt = time.perf_counter() - t0
    return {"value": ((4 * tile) ** 2 / 1e6) / dt, "unit": "output MPix/s", "cores": threads, "kind": "port",
            "cpu_model": cpu_model_name(), "seconds_per_tile": dt,
            "sample": f"CPU oracle (PyTorch fp32 restatement of the reference eval path) on one {tile}x{tile} LR tile -> "
                      f"{4 * tile}x{4 * tile} (the GPU step's own workload), 1 warm-up on 64x64 + 1 timed tile, {dt:.1f} s wall on "
                      f"{threads} threads"}


def training_side_block(dev, steps: int, with_cpu: bool, threads: int):
    """SIDE BLOCK (not the headline): the fusion-only training step of BASELINE config 5 -- batch 16 x 64 x 64 LR, experts
    precomputed, train-mode forward + L1 + backward + clip + AdamW + EMA (reference train.py:308-356) -- in ms per step on this
    GPU, beside the CPU oracle's step time (torch.autograd on the oracle's train-mode restatement) on a bounded sample."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from train_inputs import make_train_batch
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    B, S = 16, 64
    sd = synth_state_dict(SEED, parts=("fusion", "collab"))
    d = {k: torch.from_numpy(v).to(dev) for k, v in make_train_batch(503, B, S, S).items()}
    outs = {k: d["out_" + k] for k in ("hat", "dat", "nafnet")}
    feats = {k: d["feat_" + k] for k in ("hat", "dat", "nafnet")}
    tr = FusionTrainer(sd, dev)
    for _ in range(2):
        tr.step(d["lr"], d["hr"], outs, feats)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = tr.step(d["lr"], d["hr"], outs, feats)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    blk = {"workload": f"fusion-only training step, batch {B} x {S}x{S} LR -> {4 * S}x{4 * S}, cached-expert inputs, 222 trainable tensors / 940 425 values "
                       "(BASELINE configs[4]; one GPU: no gradient all-reduce in this number)",
           "ms_per_step": ms, "samples_per_s": B / (ms * 1e-3), "contraction": tr.gemm, "loss_after_warmup": float(loss),
           "peak_hbm_GiB": torch.cuda.max_memory_allocated(dev) / 2 ** 30}
    del tr
    torch.cuda.empty_cache()
    if with_cpu:
        from oracle import freqfusion_oracle as O
        from isr2_amd.train import trainable_names
        torch.set_num_threads(threads)
        Bc = 4                                             # bounded sample: a quarter of the batch, same patch size
        dc = {k: torch.from_numpy(v) for k, v in make_train_batch(503, Bc, S, S).items()}
        names = trainable_names(sd)
        args_ = (sd, dc["lr"], dc["hr"], {k: dc["out_" + k] for k in ("hat", "dat", "nafnet")}, {k: dc["feat_" + k] for k in ("hat", "dat", "nafnet")}, names)
        t0 = time.perf_counter()
        O.train_loss_and_grads(*args_)
        dt = time.perf_counter() - t0
        blk["cpu_baseline"] = {"seconds_per_sample": dt / Bc, "samples_per_s": Bc / dt, "cores": threads, "kind": "port",
                               "sample": f"oracle train-mode forward + L1 + torch.autograd backward (no optimizer) on a batch of {Bc} x {S}x{S} "
                                         f"(a quarter of the GPU step's batch), {dt:.1f} s on {threads} threads"}
        blk["speedup_vs_cpu_per_sample"] = blk["samples_per_s"] / blk["cpu_baseline"]["samples_per_s"]
    return blk


def csrc_fingerprint() -> str:
    """Content hash of the kernel sources: a PMC traffic file is only quoted while it describes these kernels."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "image-super-resolution-2_amd", "csrc")
    for f in sorted(os.listdir(d)):
        h.update(f.encode())
        h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def golden_samples(model, dev):
    """(this model's output, the REFERENCE's output) on bench tile 100 at the 65 536 sample positions of the committed golden
    tests/golden/t256_nat.npz (generated from the imported reference); None without the file."""
    path = os.path.join(ROOT, "tests", "golden", "t256_nat.npz")
    if not os.path.exists(path):
        return None
    g = np.load(path)
    out = model(torch.from_numpy(g["lr"]).to(dev)).reshape(-1).cpu()
    return out[torch.from_numpy(g["big/final/idx"])].double().numpy(), g["big/final/val"].astype(np.float64)


def golden_psnr(model, dev):
    """PSNR of this model's output against the REFERENCE's output on bench tile 100."""
    s = golden_samples(model, dev)
    if s is None:
        return None
    return 10.0 * float(np.log10(1.0 / max(float(((s[0] - s[1]) ** 2).mean()), 1e-30)))


def delta_psnr_vs_ground_truth(got, ref):
    """The north-star bar is stated on PSNR against GROUND TRUTH: |PSNR(build, GT) - PSNR(reference, GT)| <= 0.01 dB.  No real HR image
    or trained checkpoint exists offline, so the ground truth is synthesised at the operating points a x4 SR model works at:
    GT = reference output + seeded Gaussian residual of the power that puts PSNR(reference, GT) at 25 / 30 / 35 / 40 dB (a trained
    FreqFusion scores ~30 dB on DIV2K-val).  Reported per point: the measured delta on the 65 536 golden
    samples, and the closed form for an error uncorrelated with the residual, 10 log10(1 + MSE_err / MSE_residual)."""
    err = got - ref
    mse_e = float((err ** 2).mean())
    rng = np.random.Generator(np.random.Philox(2026))
    rows = {}
    for p_ref in (25.0, 30.0, 35.0, 40.0):
        sig2 = 10.0 ** (-p_ref / 10.0)
        gt = ref + rng.standard_normal(ref.shape) * np.sqrt(sig2)
        ps_ref = 10.0 * np.log10(1.0 / float(((ref - gt) ** 2).mean()))
        ps_got = 10.0 * np.log10(1.0 / float(((got - gt) ** 2).mean()))
        rows[f"{p_ref:.0f}dB"] = {"psnr_reference_vs_gt": ps_ref, "psnr_build_vs_gt": ps_got, "delta_dB": ps_got - ps_ref,
                                  "uncorrelated_error_formula_dB": -10.0 * np.log10(1.0 + mse_e / sig2)}
    return {"mse_build_vs_reference": mse_e, "points": rows,
            "worst_abs_delta_dB": max(abs(r["delta_dB"]) for r in rows.values()), "bar_dB": 0.01}


def time_mode(mode: str, sd, dev, lr, steps: int):
    """ms per step (HIP-graph replay, two lanes) and golden PSNR of another contraction mode, for the `extra` block."""
    from isr2_amd import ops
    from isr2_amd.model import FreqFusionHIP
    old = ops.gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        m = FreqFusionHIP(sd, dev)
        psnr = golden_psnr(m, dev) if tuple(lr.shape[-2:]) == (TILE, TILE) else None
        for i in range(4):                                   # same launch path as the headline: two tiles in flight on two lanes
            m.graphed_async(lr, i & 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            m.graphed_async(lr, i & 1)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / steps
        del m
        torch.cuda.empty_cache()
    finally:
        ops.set_gemm_mode(old)
    return {"ms_per_step": ms, "output_MPix_s": (4 * lr.shape[-1]) ** 2 / 1e6 / (ms * 1e-3), "psnr_vs_reference_golden_dB": psnr}


DTYPE_NAMES = {"f32": "f32 (exact fp32 MFMA)", "bf16": "bf16 (bf16 MFMA operands, fp32 accumulate, fp32 activations in HBM)", "bf16x2": "bf16x2",
               "bf16x3": "bf16x3 (split bf16 MFMA, fp32 accumulate, fp32-grade results)"}


def self_spawn(args) -> int:
    """`python bench.py --gpus N` called plainly: start N fresh ranks of this script (no GPU call has happened in this process)."""
    from isr2_amd.parallel import spawn_ranks, visible_gpu_count
    ndev = visible_gpu_count()                                # sysfs / visibility lists: the parent makes no HIP call at all
    if os.environ.get("FF_DIST_BACKEND", "nccl") == "nccl" and 0 <= ndev < args.gpus:
        print(f"bench.py: --gpus {args.gpus} but only {ndev} GPU(s) visible on this node (one rank per GPU over RCCL)", file=sys.stderr)
        return 2
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    return spawn_ranks(cmd, args.gpus)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-graph", action="store_true", help="time the eager Python launch loop instead of HIP-graph replay")
    ap.add_argument("--lanes", type=int, default=int(os.environ.get("FF_BENCH_LANES", "2")), choices=(1, 2),
                    help="tiles in flight: 2 = consecutive steps replay on two lane streams (model.graphed_async, the plugin's tile pipeline), 1 = strictly one after the other")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what the headline does not need: per-kernel accounting and roofline, "
                         "the other contraction modes and accuracy against the reference, the CPU baseline, the training side block")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle baselines")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the other contraction modes, the accuracy block and the training side block")
    ap.add_argument("--no-train", action="store_true", help="with --full: skip the training-step side block (BASELINE configs[4])")
    ap.add_argument("--tile", type=int, default=TILE)
    ap.add_argument("--dtype", default=os.environ.get("FF_GEMM", "bf16"), choices=("bf16", "bf16x3", "f32"),
                    help="contraction mode of the headline run.  BASELINE configs[1] names bf16: plain bf16 MFMA operands with fp32 "
                         "accumulation (68.8 dB against the reference's output; a --full line carries the PSNR-vs-ground-truth deltas); "
                         "bf16x3 = fp32-grade split-bf16 products (123 dB), the plugin's default; f32 = exact fp32 MFMA")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's SR output to DIR/sr.npy (float32; DIR/sr_rank<r>.npy per rank when --gpus > 1)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_spawn(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    # one rank per GPU.  (Rehearsal on a box with fewer GPUs than ranks: FF_DIST_BACKEND=gloo lets several ranks share a
    # card -- RCCL refuses that -- so the whole N>1 code path can be exercised on one MI355X; never used for a result.)
    backend = os.environ.get("FF_DIST_BACKEND", "nccl")
    ndev = max(torch.cuda.device_count(), 1)
    if backend == "nccl" and world > ndev:
        raise SystemExit(f"bench.py: {world} ranks but only {ndev} GPUs visible (one rank per GPU over RCCL)")
    dev = torch.device(f"cuda:{local_rank % ndev}")
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from isr2_amd import ops
    from isr2_amd.model import FreqFusionHIP
    ops.set_gemm_mode(args.dtype)

    log("generating / broadcasting weights")
    sd, bcast_s = broadcast_weights(rank, world, dev)
    model = FreqFusionHIP(sd, dev)
    log("model ready")
    tile = args.tile
    lr = make_tile(100 + rank, tile).to(dev)                # a different resident tile per rank
    flop_per_tile = FLOP_PER_TILE * (tile / TILE) ** 2
    mpix_per_tile = (4 * tile) ** 2 / 1e6

    # ---- warm-up (also fills the caching allocator and the twiddle caches), then optional graph capture -------
    t_e = time.perf_counter()
    out = model(lr)
    torch.cuda.synchronize()
    log(f"first eager forward {time.perf_counter() - t_e:.2f} s")
    t_e = time.perf_counter()
    out = model(lr)
    torch.cuda.synchronize()
    log(f"second eager forward {time.perf_counter() - t_e:.3f} s")
    use_graph = not args.no_graph
    graph = None
    if use_graph:
        try:
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                model(lr)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = model(lr)
            torch.cuda.synchronize()
            log("graph captured")
        except Exception as e:                               # capture is an optimisation of the launch path only
            print(f"[bench] graph capture failed ({type(e).__name__}: {e}); timing the eager loop", file=sys.stderr)
            graph = None
            torch.cuda.synchronize()

    lanes = args.lanes if graph is not None else 1
    if lanes == 2:
        try:                                                 # capture both lane graphs outside the timed region
            model.graphed_async(lr, 0)
            model.graphed_async(lr, 1)
            torch.cuda.synchronize()
            log("two lane graphs captured")
        except Exception as e:
            print(f"[bench] lane capture failed ({type(e).__name__}: {e}); one tile at a time", file=sys.stderr)
            lanes = 1
            torch.cuda.synchronize()
    nstep = [0]
    last = [None]                                            # the output tensor of the latest step

    def step():
        if lanes == 2:                                       # step i on lane i & 1: step i+1 starts while step i drains
            last[0] = model.graphed_async(lr, nstep[0] & 1)[0]
            nstep[0] += 1
        elif graph is not None:
            graph.replay()
            last[0] = out
        else:
            last[0] = model(lr)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    log(f"timed region: {args.steps} steps in {elapsed:.3f} s")
    if world > 1:
        tmax = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    if args.dump_outputs:                                    # before any other pass can touch the step's output buffer
        os.makedirs(args.dump_outputs, exist_ok=True)
        dump = os.path.join(args.dump_outputs, "sr.npy" if world == 1 else f"sr_rank{rank}.npy")
        sr = last[0].detach().float().cpu().numpy()
        if sr.nbytes > DUMP_MAX_BYTES:                       # large --tile: a fixed seeded sample of the output, same positions every run
            idx = np.sort(np.random.default_rng(SEED).choice(sr.size, DUMP_MAX_BYTES // 4, replace=False))
            sr = sr.reshape(-1)[idx]
        np.save(dump, sr)
        log(f"last step's output {tuple(last[0].shape)} written to {dump}")

    # ---- --full only from here on: what the headline does not need ------------------------------------------
    # per-kernel-class accounting: one extra eager pass with HIP events around every launch
    roof, breakdown, stages = None, None, None
    if rank == 0 and args.full:
        def _timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            torch.cuda.synchronize()
            return r, e0.elapsed_time(e1)
        hat_o, t_hat = _timed(lambda: model.hat.forward(lr))
        dat_o, t_dat = _timed(lambda: model.dat.forward(lr))
        naf_o, t_naf = _timed(lambda: model.nafnet.forward(lr))
        _, t_fus = _timed(lambda: model.fusion.forward(lr, {"hat": hat_o, "dat": dat_o, "nafnet": naf_o}))
        stages = {"hat_ms": round(t_hat, 2), "dat_ms": round(t_dat, 2), "nafnet_ms": round(t_naf, 2), "fusion_ms": round(t_fus, 2),
                  "note": "eager launches (includes Python launch gaps the graph replay does not have)"}
        ms_flag = model.multi_stream
        model.multi_stream = False                      # per-kernel durations in isolation: no other stream sharing the CUs
        try:
            with ops.profile() as prof:
                model(lr)
        finally:
            model.multi_stream = ms_flag
        agg = {}
        for name, ms, fl, by in prof.records():
            a = agg.setdefault(name, [0, 0.0, 0.0, 0.0])
            a[0] += 1; a[1] += ms; a[2] += fl; a[3] += by
        mf = [agg.get(k, [0, 0.0, 0.0, 0.0]) for k in ("conv2d", "linear")]
        n_l, ms_l, fl_l = mf[0][0] + mf[1][0], mf[0][1] + mf[1][1], mf[0][2] + mf[1][2]
        achieved = fl_l / (ms_l * 1e-3) / 1e12 if ms_l > 0 else 0.0
        mode = ops.gemm_mode()
        peak = PEAK_TF[mode]
        traffic, tnote = None, "no PMC profile committed"
        def _ver(f):
            m = re.search(r"_v(\d+)\.json$", f)
            return int(m.group(1)) if m else -1
        tfiles = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic_v*.json")), key=lambda f: (os.path.basename(f)[:3], _ver(f)))
        tdoc = None
        fp = csrc_fingerprint()
        if tfiles:                                      # PMC counters come from separate rocprofv3 passes (tools/pmc_traffic.py)
            tdoc = json.load(open(tfiles[-1]))
            if tdoc.get("csrc_fingerprint") != fp:      # the counters describe other kernels than the ones just timed
                tnote = (f"profiles/{os.path.basename(tfiles[-1])} was collected for csrc {tdoc.get('csrc_fingerprint')}, the "
                         f"kernels timed here are {fp}: stale, not quoted")
                tdoc = None
            else:
                traffic = tdoc["conv_igemm_all_variants"]["hbm_MB_per_launch"] * 1e6
                tnote = ("HBM bytes per launch, (2*FETCH_SIZE+WRITE_SIZE)*1024 from profiles/" + os.path.basename(tfiles[-1])
                         + f" (csrc {fp}, git {tdoc.get('git', 'n/a')})")
        roof = {"bound": "mfma", "kernel": "ff_conv2d*: conv_igemm_bf16_kernel (all tile variants) + conv3x3_halo_kernel (f32 mode: conv_igemm_kernel) -- every Conv2d and every Linear with K > 192",
                "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                "traffic": traffic, "traffic_note": tnote,
                "algorithmic_bytes_per_launch": 1e6 * (mf[0][3] + mf[1][3]) / max(n_l, 1) / 1e6,
                "mfma_flops_per_algorithmic_flop": MFMA_PER_ALGO_FLOP[mode], "executed_mfma_frac": achieved * MFMA_PER_ALGO_FLOP[mode] / peak,
                "launches_per_tile": n_l, "avg_launch_us": 1e3 * ms_l / max(n_l, 1),
                "algorithmic_gflop_per_launch": fl_l / max(n_l, 1) / 1e9,
                "share_of_tile_time": ms_l / max(sum(a[1] for a in agg.values()), 1e-9)}
        # the two other large kernel families, against the roofline that bounds each (same HIP-event accounting)
        def _fam(name, bound, peak_v, unit, key):
            a = agg.get(name)
            if not a or a[1] <= 0:
                return None
            ach = (a[3] / (a[1] * 1e-3) / 1e9) if bound == "hbm" else (a[2] / (a[1] * 1e-3) / 1e12)
            tr = tdoc[key]["hbm_MB_per_launch"] * 1e6 if tdoc and key in tdoc else None
            return {"kernel": name, "bound": bound, "achieved": ach, "peak": peak_v, "unit": unit, "frac": ach / peak_v,
                    "traffic": tr, "launches_per_tile": a[0], "avg_launch_us": 1e3 * a[1] / a[0],
                    "algorithmic_bytes_per_launch": a[3] / a[0], "algorithmic_gflop_per_launch": a[2] / a[0] / 1e9}
        hbm_gb = None
        if tdoc and tdoc.get("forwards"):
            hbm_gb = tdoc["whole_forward"]["hbm_MB_total"] / tdoc["forwards"] / 1e3
        step_s = elapsed / args.steps
        roof["whole_path"] = {"hbm_GB_per_tile": hbm_gb, "TB_s": (hbm_gb / 1e3 / step_s) if hbm_gb else None,
                              "algorithmic_TFLOPs": flop_per_tile / step_s / 1e12,
                              "compulsory_GB": 0.689 + 4 * 3 * (tile * tile + 16 * tile * tile) / 1e9,
                              "note": "hbm_GB_per_tile = PMC (2*FETCH_SIZE+WRITE_SIZE) summed over every kernel of one forward; "
                                      "compulsory = fp32 weights read once + LR in + SR out"}
        # the conv / GEMM family launch by launch against the bound that applies to EACH launch: algorithmic intensity above the ridge
        # (executable MFMA peak / HBM peak) -> MFMA-bound, below -> HBM-bound (NAFNet's 1x1 convolutions at 64 / 128 channels, the
        # 3- and 9-channel heads of the fusion stack); the family entry above stays the undivided total
        ridge = (peak / MFMA_PER_ALGO_FLOP[mode]) * 1e12 / 8e12
        sub = {"mfma": [0, 0.0, 0.0, 0.0], "hbm": [0, 0.0, 0.0, 0.0]}
        for name, ms, fl, by in prof.records():
            if name in ("conv2d", "linear") and by > 0:
                a = sub["mfma" if fl / by >= ridge else "hbm"]
                a[0] += 1; a[1] += ms; a[2] += fl; a[3] += by
        roof["by_launch_bound"] = {
            "ridge_flop_per_byte": ridge,
            "mfma_bound": {"launches_per_tile": sub["mfma"][0], "ms_per_tile": sub["mfma"][1],
                           "achieved_TFLOPs": sub["mfma"][2] / max(sub["mfma"][1], 1e-9) / 1e9,
                           "frac_of_peak": sub["mfma"][2] / max(sub["mfma"][1], 1e-9) / 1e9 / peak,
                           "executed_mfma_frac": sub["mfma"][2] / max(sub["mfma"][1], 1e-9) / 1e9 * MFMA_PER_ALGO_FLOP[mode] / peak},
            "hbm_bound": {"launches_per_tile": sub["hbm"][0], "ms_per_tile": sub["hbm"][1],
                          "achieved_GBs": sub["hbm"][3] / max(sub["hbm"][1], 1e-9) / 1e6,
                          "frac_of_peak": sub["hbm"][3] / max(sub["hbm"][1], 1e-9) / 1e6 / 8000.0},
            "note": "algorithmic FLOPs / algorithmic bytes per launch, HIP-event durations of the same single-stream pass"}
        roof["other_kernels"] = [r for r in (
            _fam("token_linear", "hbm", 8000.0, "GB/s", "token_linear_all_variants"),
            _fam("win_attn_fused", "mfma", peak, "TFLOP/s", "win_attn_fused_all_variants"),
            _fam("token_projmlp", "mfma", peak, "TFLOP/s", "token_projmlp"),
            _fam("window_attn", "mfma", peak, "TFLOP/s", "window_attn_all_variants"),
            _fam("token_mlp", "mfma", peak, "TFLOP/s", "token_mlp")) if r]
        breakdown = {k: {"launches": v[0], "ms": round(v[1], 3), "tflops": round(v[2] / max(v[1], 1e-9) / 1e9, 2),
                         "gbps": round(v[3] / max(v[1], 1e-9) / 1e6, 1)} for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1])}

    if rank == 0:
        value = world * args.steps * mpix_per_tile / elapsed
        line = {
            "metric": "output MPix/s at x4 SR (256->1024)", "value": value, "unit": "output MPix/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": DTYPE_NAMES[ops.gemm_mode()], "data": "synthetic",
            "config": {"workload": f"FreqFusion x4 full 3-expert forward (HAT-L + DAT + NAFNet-SR + fusion stack), one "
                                   f"{tile}x{tile} LR tile -> {4 * tile}x{4 * tile} per step per GPU (BASELINE configs[1]); "
                                   "seeded synthetic weights (172.3 M params), 1/f-noise tiles",
                       "tile": tile, "tiles_per_step_per_gpu": 1,
                       "parallelism": f"tile-sharded x{world}, weights {'RCCL' if backend == 'nccl' else backend + ' (rehearsal)'}-broadcast once ({bcast_s * 1e3:.1f} ms), no per-tile collectives",
                       "launch": "hipGraph replay" if graph is not None else "eager",
                       "tiles_in_flight": lanes},
            "path_tflops": world * args.steps * flop_per_tile / elapsed / 1e12,
        }
        if args.full:
            line.update({"roofline": roof, "stage_ms_per_tile": stages, "kernel_breakdown_ms_per_tile": breakdown})
        if args.full and world == 1 and not args.no_extra:
            log("side measurements: f32 and plain-bf16 contraction modes")
            one_ms = None
            if lanes == 2:                                   # the same tile strictly one after the other (latency of one tile)
                for _ in range(2):
                    graph.replay()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(args.steps):
                    graph.replay()
                torch.cuda.synchronize()
                one_ms = 1e3 * (time.perf_counter() - t1) / args.steps
            gs = golden_samples(model, dev) if tile == TILE else None
            extra = {"note": "same workload and launch path in the other contraction modes; PSNR is against the REFERENCE's output "
                             "on bench tile 100 (tests/golden/t256_nat.npz)",
                     "one_tile_at_a_time_ms": one_ms,
                     ops.gemm_mode(): {"ms_per_step": line["ms_per_step"], "output_MPix_s": value,
                                       "psnr_vs_reference_golden_dB": (10.0 * float(np.log10(1.0 / max(float(((gs[0] - gs[1]) ** 2).mean()), 1e-30)))) if gs else None}}
            if gs:
                line["accuracy"] = {"psnr_vs_reference_output_dB": extra[ops.gemm_mode()]["psnr_vs_reference_golden_dB"],
                                    "delta_psnr_vs_ground_truth": delta_psnr_vs_ground_truth(*gs)}
            for mode in ("bf16x3", "f32", "bf16"):
                if mode != ops.gemm_mode():
                    extra[mode] = time_mode(mode, sd, dev, lr, max(2, min(args.steps, 5)))
            line["extra"] = extra
        if args.full and world == 1 and not args.no_cpu_baseline:
            log(f"cpu baseline (oracle, {tile}x{tile} tile, {host_threads()} threads)")
            line["cpu_baseline"] = cpu_baseline(sd, host_threads(), tile)
        if args.full and world == 1 and not args.no_train and not args.no_extra:
            log("side block: fusion-only training step (config 5)")
            del model
            torch.cuda.empty_cache()
            try:
                line["training_step"] = training_side_block(dev, max(2, min(args.steps, 5)), not args.no_cpu_baseline, host_threads())
            except Exception as e:                               # the side block never takes the headline down
                line["training_step"] = {"error": f"{type(e).__name__}: {e}"}
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
