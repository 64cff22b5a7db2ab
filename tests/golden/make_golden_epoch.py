"""Fixtures of the epoch driver (gradient accumulation, learning-rate schedule, validation with EMA weights), generated from the
IMPORTED reference (build container only; only the arrays below are committed).

    python tests/golden/make_golden_epoch.py lr          # lr_schedule.json                 (instant)
    python tests/golden/make_golden_epoch.py accum       # train_accum_b2_16.npz            (~1 min)
    python tests/golden/make_golden_epoch.py stage3      # train_accum_stage3_b2_16.npz     (seconds)
    python tests/golden/make_golden_epoch.py validate    # validate_b1_16.npz               (seconds)

lr: torch's own CosineAnnealingWarmRestarts(T_0 50, T_mult 2, eta_min 5e-8) on an AdamW group of lr 1.5e-4, driven in the ORDER of
the reference's epoch loop: warmup_lr() writes the group's lr while epoch < 5 (train.py:1063-1065), the epoch trains at whatever the
group holds, scheduler.step() runs after the epoch only when epoch >= 5 (:1105-1107).  So epoch 5 still trains at epoch 4's warm-up
value and the first restart lands on epoch 55.

accum: train_epoch_cached (train.py:306-356) restated with accumulation_steps = 2 on five micro-batches B = 2, 16x16
(make_train_batch seeds 511..515) per epoch, epochs 5 and 6 in this fixed order, no augmentation, dropout 0, gradient_clip 0.05 (so
that the clip IS active on the accumulated gradient; with 1.0 it never engages at this size), lr of the epoch from the list above.
The fifth micro-batch of each epoch is the window the reference discards (optimizer.zero_grad() at the top of the next epoch).
Stored: per micro-batch the UNSCALED loss; after the first window every gradient and its pre-clip norm; the pre-clip norm of all four
windows; BatchNorm buffers after each epoch; parameters and EMA shadow after the 4 optimizer steps.  Tensors are stored as
make_golden_losses.pack does (L2 norm + the whole tensor up to FULL_MAX values, else NS values at make_golden_train.sidx positions,
which the test re-derives from the tensor's name).

stage3: the first window again with the stage-3 weights {l1 .60, swt .25, fft .10, ssim .05} (make_golden_losses' components).

validate: validate_epoch (train.py:413-523) in cached mode: parameters synth_state_dict(1234), EMA shadow overwritten with
synth_state_dict(4321)'s values for every shadow tensor that dict holds, ema.apply -> eval forward_with_precomputed (B = 1 per call)
-> clamp -> MetricCalculator(crop_border 4, test_y_channel True) -> ema.restore; and the same with EMA off.
"""
import os
import sys
import json
import math
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_train import build_cached_mode_model, sidx, HP  # noqa: E402
from train_inputs import make_train_batch  # noqa: E402

SCHED = dict(base_lr=1.5e-4, warmup_epochs=5, warmup_lr=5e-7, T_0=50, T_mult=2, eta_min=5e-8)     # configs/train_config.yaml:102-120
FULL_MAX, NS = 256, 256
ACCUM, CLIP, EPOCHS, SEEDS = 2, 0.05, (5, 6), (511, 512, 513, 514, 515)
STAGE3 = {"l1": 0.60, "swt": 0.25, "fft": 0.10, "ssim": 0.05}


def driven_lrs(n_epochs, **kw):
    """The lr each epoch trains at: torch's scheduler and the warm-up in the order of the reference's loop."""
    c = dict(SCHED, **kw)
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=c["base_lr"])
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=c["T_0"], T_mult=c["T_mult"], eta_min=c["eta_min"])
    out = []
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for epoch in range(n_epochs):
            if epoch < c["warmup_epochs"]:                                                         # train.py:119-125
                lr = c["warmup_lr"] + (c["base_lr"] - c["warmup_lr"]) * epoch / c["warmup_epochs"]
                for g in opt.param_groups:
                    g["lr"] = lr
            out.append(float(opt.param_groups[0]["lr"]))
            if epoch >= c["warmup_epochs"]:
                sched.step()
    return out


def make_lr():
    lrs = driven_lrs(400)
    json.dump({"config": SCHED, "lr": lrs}, open(os.path.join(HERE, "lr_schedule.json"), "w"))
    print("lr_schedule.json: epochs 4/5/6/54/55 =", [f"{lrs[e]:.6e}" for e in (4, 5, 6, 54, 55)])


def compact(name, t):
    f = t.detach().float().reshape(-1).numpy()
    l2 = float(np.sqrt((f.astype(np.float64) ** 2).sum()))
    return l2, (f if f.size <= FULL_MAX else f[sidx(name, f.size, NS)]).astype(np.float32)


def pack(blob, kind, items):
    rows = [(n,) + compact(n, t) for n, t in items]
    blob[f"{kind}/names"] = np.array(json.dumps([r[0] for r in rows]))
    blob[f"{kind}/l2"] = np.array([r[1] for r in rows], dtype=np.float64)
    blob[f"{kind}/count"] = np.array([r[2].size for r in rows], dtype=np.int32)
    blob[f"{kind}/vals"] = np.concatenate([r[2] for r in rows])


def batches():
    out = []
    for s in SEEDS:
        d = {k: torch.from_numpy(v) for k, v in make_train_batch(s, 2, 16, 16).items()}
        out.append((d["lr"], d["hr"], {k: d["out_" + k] for k in ("hat", "dat", "nafnet")}, {k: d["feat_" + k] for k in ("hat", "dat", "nafnet")}))
    return out


def run_accum(stage3=False):
    torch.manual_seed(0)
    model, sd, live_missing = build_cached_mode_model()
    model.train()
    if stage3:
        from make_golden_losses import reference_losses, combined
        crit = reference_losses()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    hp = dict(HP, clip=CLIP)
    opt = torch.optim.AdamW(model.parameters(), lr=hp["lr"], betas=hp["betas"], weight_decay=hp["weight_decay"], eps=hp["eps"])
    from src.utils.checkpoint_manager import EMAModel
    ema = EMAModel(model, decay=hp["ema_decay"])
    lrs = driven_lrs(max(EPOCHS) + 1)
    data = batches()
    epochs = EPOCHS[:1] if stage3 else EPOCHS
    data = data[:ACCUM] if stage3 else data
    blob = {"meta": np.array(json.dumps({"B": 2, "h": 16, "w": 16, "input_seeds": list(SEEDS[:len(data)]), "weight_seed": 1234, "hp": hp,
                                         "accumulation_steps": ACCUM, "epochs": list(epochs), "lr": [lrs[e] for e in epochs], "dropout": 0.0,
                                         "loss_weights": STAGE3 if stage3 else {"l1": 1.0}, "full_max": FULL_MAX, "ns": NS,
                                         "dead_parameters_not_in_synth": live_missing}))}
    losses, norms, comps_all, steps = [], [], [], 0
    for epoch in epochs:
        for g in opt.param_groups:
            g["lr"] = lrs[epoch]
        opt.zero_grad()                                                                            # train.py:306
        for bi, (lr, hr, outs, feats) in enumerate(data):
            t0 = time.time()
            sr = model.forward_with_precomputed(lr, outs, feats).clamp(0, 1)
            if stage3:
                loss, comps = combined(crit, STAGE3, sr, hr)
                comps_all.append({k: float(v) for k, v in comps.items()})
            else:
                loss = (sr - hr).abs().mean()
            (loss / ACCUM).backward()                                                              # train.py:330-334
            losses.append(float(loss))
            if (bi + 1) % ACCUM == 0:
                if steps == 0:
                    blob["nograd"] = np.array(json.dumps([n for n, p in named if p.grad is None]))
                    pack(blob, "grad", [(n, p.grad) for n, p in named if p.grad is not None])
                gn = torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP)
                opt.step()
                opt.zero_grad()
                ema.update(model)
                norms.append(float(gn))
                steps += 1
            print(f"epoch {epoch} micro-batch {bi}: loss {float(loss):.6f}  windows done {steps}  last norm {norms[-1] if norms else None}  ({time.time() - t0:.1f} s)", flush=True)
        for n, b in model.named_buffers():
            if n.endswith(("running_mean", "running_var", "num_batches_tracked")):
                blob[f"bn_e{epoch}/" + n] = b.detach().numpy().copy()
    blob["losses"] = np.array(losses, dtype=np.float64)
    blob["grad_norms"] = np.array(norms, dtype=np.float64)
    if stage3:
        blob["components"] = np.array(json.dumps(comps_all))
    pack(blob, f"param{steps}", [(n, p.data) for n, p in named])
    pack(blob, f"ema{steps}", [(n, ema.shadow[n]) for n, _ in named])
    fname = "train_accum_stage3_b2_16.npz" if stage3 else "train_accum_b2_16.npz"
    np.savez_compressed(os.path.join(HERE, fname), **blob)
    size = os.path.getsize(os.path.join(HERE, fname))
    print("wrote", fname, size // 1024, "KiB; steps", steps, "norms", norms, flush=True)
    assert size < (1 << 20), size
    assert norms[0] > CLIP, "the clip must be active on the first window"


def make_validate():
    from isr2_amd.weights import synth_state_dict
    torch.manual_seed(0)
    model, sd, _ = build_cached_mode_model()
    from src.utils.checkpoint_manager import EMAModel
    from src.utils import MetricCalculator
    ema = EMAModel(model, decay=HP["ema_decay"])
    other = synth_state_dict(4321, parts=("fusion", "collab"))
    taken = [k for k in ema.shadow if k in other]
    for k in taken:
        assert tuple(other[k].shape) == tuple(ema.shadow[k].shape), k
        ema.shadow[k] = other[k].float().clone()
    d = {k: torch.from_numpy(v) for k, v in make_train_batch(521, 2, 16, 16).items()}
    samples = []
    for b in range(2):
        samples.append((d["lr"][b:b + 1], d["hr"][b:b + 1], {k: d["out_" + k][b:b + 1] for k in ("hat", "dat", "nafnet")},
                        {k: d["feat_" + k][b:b + 1] for k in ("hat", "dat", "nafnet")}))
    from src.utils.metrics import calculate_psnr, calculate_ssim

    @torch.no_grad()
    def run(use_ema):
        model.eval()
        if use_ema:
            backup = ema.save(model)
            ema.apply(model)
        calc = MetricCalculator(crop_border=4, test_y_channel=True)
        srs, per = [], []
        for lr, hr, outs, feats in samples:
            sr = model.forward_with_precomputed(lr, outs, feats).clamp(0, 1)
            calc.update(sr, hr)
            per.append((calculate_psnr(sr[0], hr[0], 4, True), calculate_ssim(sr[0], hr[0], 4, True)))
            srs.append(sr[0].numpy().copy())
        if use_ema:
            ema.restore(model, backup)
        return np.stack(srs), np.array(per, dtype=np.float64), calc.get_metrics()

    before = {k: v.clone() for k, v in model.state_dict().items()}
    sr_on, per_on, m_on = run(True)
    sr_off, per_off, m_off = run(False)
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    diff = float(np.abs(sr_on - sr_off).max())
    assert diff > 1e-2 and abs(m_on["psnr"] - m_off["psnr"]) > 0.1, (diff, m_on, m_off)        # or the fixture proves nothing
    blob = {"meta": np.array(json.dumps({"input_seed": 521, "weight_seed": 1234, "ema_seed": 4321, "h": 16, "w": 16, "crop_border": 4,
                                         "test_y_channel": True, "shadow_tensors": len(ema.shadow), "shadow_taken": len(taken)})),
            "sr_ema": sr_on.astype(np.float32), "sr_model": sr_off.astype(np.float32), "per_image_ema": per_on, "per_image_model": per_off,
            "mean_ema": np.array([m_on["psnr"], m_on["ssim"]]), "mean_model": np.array([m_off["psnr"], m_off["ssim"]])}
    np.savez_compressed(os.path.join(HERE, "validate_b1_16.npz"), **blob)
    print(f"validate_b1_16.npz: {len(taken)} of {len(ema.shadow)} shadow tensors replaced; EMA on {m_on}, off {m_off}, max |sr_on - sr_off| {diff:.4f}",
          os.path.getsize(os.path.join(HERE, "validate_b1_16.npz")) // 1024, "KiB")
    assert all(math.isfinite(v) for v in per_on.reshape(-1))


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("FF_THREADS", "8")))
    for a in (sys.argv[1:] or ["lr", "accum", "stage3", "validate"]):
        {"lr": make_lr, "accum": run_accum, "stage3": lambda: run_accum(True), "validate": make_validate}[a]()
