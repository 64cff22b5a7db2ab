"""Fixtures of the reference's staged training losses (src/losses/perceptual_loss.py, CombinedLoss.forward :1207-1283), generated from
the IMPORTED reference (build container only; only the arrays below are committed).

    python tests/golden/make_golden_losses.py losses     # losses.npz            (seconds)
    python tests/golden/make_golden_losses.py stages     # loss_stages.json      (get_loss_stage on configs/train_config.yaml)
    python tests/golden/make_golden_losses.py b2 b4      # train_stage3_b2_16.npz, train_stage3_b4_32.npz (~1 min)

The two training fixtures hold make_golden_train's quantities (loss, components, gradient norms, every gradient after the first
backward, parameters and EMA shadow after 3 steps, the clamped prediction) in a compact form, since the repository keeps fixtures small:
per tensor its L2 norm and either the whole tensor (numel <= 64) or 64 values at indices that are NOT stored but re-derived from the
tensor's name (`sample_idx`, a seeded draw); 4096 such values of `sr`.  The tensors of one kind are packed into a few arrays
(`pack`: `<kind>/names` JSON, `<kind>/l2`, `<kind>/count`, `<kind>/vals` concatenated in name order) -- one archive member per
tensor would cost more in zip headers than the values themselves.  BatchNorm statistics are not stored: the stage-3 forward is
the stage-1 one, pinned by train_*.npz.

The loss module imports torchvision unguarded and SWT needs PyWavelets; neither is installed, so two more sys.modules stubs are
registered: `torchvision.models` (empty: VGG is never built) and `pywt.Wavelet('haar')` carrying PyWavelets' haar decomposition
filters.  CombinedLoss.__init__ builds a VGG19, so the components are instantiated one by one exactly as it does (:1118-1142) and
its weighted sum is restated in its order.

losses.npz, per case k (pred seeded in [-0.05, 1.05] so that the clamp of train.py:325 is exercised, target in [0, 1], NCHW): for
every component c, `k/c/value` and the gradient w.r.t. the PRE-clamp prediction at weight 1 -- `k/c/grad` in full (NHWC) for the
small cases, `k/c/grad_l2` + 4096 seeded NHWC samples (`k/c/idx`, `k/c/val`) for the B=16 case -- and `k/stage{1,2,3}` totals.
The inputs are regenerated from `k/meta` (numpy PCG64 is stable across platforms); `k/input_sums` pins them.
"""
import os
import sys
import json
import hashlib
import types
import contextlib
import io as _io

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_train import build_cached_mode_model, sidx, HP  # noqa: E402
from _ref_import import install_shims, REF_ROOT  # noqa: E402
from train_inputs import make_train_batch  # noqa: E402

COMPONENTS = ("l1", "charbonnier", "l2", "ssim", "edge", "fft", "swt")            # CombinedLoss.forward's order (vgg / clip: 0)
STAGES = {1: {"l1": 1.0}, 2: {"l1": 0.75, "swt": 0.20, "fft": 0.05}, 3: {"l1": 0.60, "swt": 0.25, "fft": 0.10, "ssim": 0.05}}
LOSS_CASES = {"b2_64": (2, 64, 64, 601, True), "b1_72x40": (1, 72, 40, 602, True), "b16_256": (16, 256, 256, 603, False)}
NSAMP = 4096


def loss_inputs(B, H, W, seed):
    """pred in [-0.05, 1.05], target in [0, 1]; NCHW float32 (the fixtures' own draw, repeated by the tests)."""
    rng = np.random.default_rng(seed)
    pred = (rng.random((B, 3, H, W), dtype=np.float32) * np.float32(1.1) - np.float32(0.05)).astype(np.float32)
    target = rng.random((B, 3, H, W), dtype=np.float32)
    return pred, target


def install_loss_shims():
    install_shims()
    if "torchvision" not in sys.modules:
        tv = types.ModuleType("torchvision")
        tv.models = types.ModuleType("torchvision.models")
        sys.modules["torchvision"] = tv
        sys.modules["torchvision.models"] = tv.models
    if "pywt" not in sys.modules:
        pywt = types.ModuleType("pywt")

        class Wavelet:
            _F = {"haar": ([0.7071067811865476, 0.7071067811865476], [-0.7071067811865476, 0.7071067811865476])}

            def __init__(self, name):
                self.name = name
                self.dec_lo, self.dec_hi = (list(v) for v in self._F[name])

        pywt.Wavelet = Wavelet
        sys.modules["pywt"] = pywt


def reference_losses():
    install_loss_shims()
    with contextlib.redirect_stdout(_io.StringIO()):
        from src.losses import perceptual_loss as PL
    assert PL.PYWT_AVAILABLE
    return {"l1": PL.L1Loss(), "charbonnier": PL.CharbonnierLoss(eps=1e-6), "l2": PL.L2Loss(), "ssim": PL.SSIMLoss(),
            "edge": PL.EdgeLoss(), "fft": PL.FFTLoss(focus_high_freq=True),
            "swt": PL.SWTLoss(wavelet="haar", level=2, use_gpu_approximation=True)}


def combined(crit, weights, pred, target):
    """CombinedLoss.forward's weighted sum (:1232-1276): `total = total + w * loss` for every weight > 0, in that order."""
    total = torch.tensor(0.0)
    comps = {}
    for k in COMPONENTS:
        if weights.get(k, 0) > 0:
            comps[k] = crit[k](pred, target)
            total = total + weights[k] * comps[k]
    return total, comps


def make_losses():
    crit = reference_losses()
    blob = {}
    for tag, (B, H, W, seed, full) in LOSS_CASES.items():
        pred, target = loss_inputs(B, H, W, seed)
        blob[f"{tag}/meta"] = np.array(json.dumps({"B": B, "H": H, "W": W, "seed": seed, "full": full}))
        blob[f"{tag}/input_sums"] = np.array([pred.astype(np.float64).sum(), target.astype(np.float64).sum()])
        t = torch.from_numpy(target)
        for c in COMPONENTS:
            p = torch.from_numpy(pred).requires_grad_(True)
            v = crit[c](p.clamp(0, 1), t)
            v.backward()
            g = p.grad.permute(0, 2, 3, 1).contiguous().reshape(-1).numpy()
            blob[f"{tag}/{c}/value"] = np.array(float(v), dtype=np.float64)
            blob[f"{tag}/{c}/grad_l2"] = np.array(np.sqrt((g.astype(np.float64) ** 2).sum()))
            blob[f"{tag}/{c}/grad_maxabs"] = np.array(float(np.abs(g).max()))
            if full:
                blob[f"{tag}/{c}/grad"] = g.astype(np.float32)
            else:
                idx = sidx(f"losses/{tag}/{c}", g.size, NSAMP)
                blob[f"{tag}/{c}/idx"], blob[f"{tag}/{c}/val"] = idx, g[idx].astype(np.float32)
            print(f"{tag} {c}: {float(v):.8f}  |grad| {float(blob[f'{tag}/{c}/grad_l2']):.6e}", flush=True)
        with torch.no_grad():
            for s, w in STAGES.items():
                tot, _ = combined(crit, w, torch.from_numpy(pred).clamp(0, 1), t)
                blob[f"{tag}/stage{s}"] = np.array(float(tot), dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "losses.npz"), **blob)
    print("wrote losses.npz", os.path.getsize(os.path.join(HERE, "losses.npz")) // 1024, "KiB")


def make_stages():
    install_loss_shims()
    import yaml
    with contextlib.redirect_stdout(_io.StringIO()):
        import importlib
        rtrain = importlib.import_module("train")
    cfg = yaml.safe_load(open(os.path.join(REF_ROOT, "configs", "train_config.yaml")))
    out = []
    for e in (0, 79, 80, 149, 150, 199, 200, 500):
        num, w, name = rtrain.get_loss_stage(e, cfg["loss"])
        out.append({"epoch": e, "stage": num, "weights": {k: float(v) for k, v in w.items()}, "name": name})
    json.dump(out, open(os.path.join(HERE, "loss_stages.json"), "w"), indent=1)
    print(json.dumps(out, indent=1))


TRAIN_FULL_MAX, TRAIN_NS, SR_NS = 64, 64, 4096


def sample_idx(name, numel, n):
    """The sample positions of a training-fixture tensor: a draw seeded by the tensor's name (tests re-derive them)."""
    s = int.from_bytes(hashlib.sha256(("stage3/" + name).encode()).digest()[:4], "little")
    return np.random.default_rng(s).integers(0, numel, size=n).astype(np.int64)


def compact(name, t):
    """(l2, stored values): the whole tensor when numel <= TRAIN_FULL_MAX, else TRAIN_NS values at sample_idx(name, ...)."""
    f = t.detach().float().reshape(-1).numpy()
    l2 = float(np.sqrt((f.astype(np.float64) ** 2).sum()))
    return l2, (f if f.size <= TRAIN_FULL_MAX else f[sample_idx(name, f.size, TRAIN_NS)]).astype(np.float32)


def pack(blob, kind, items):
    """items: [(name, tensor)] -> <kind>/names, <kind>/l2, <kind>/count, <kind>/vals."""
    rows = [(n,) + compact(n, t) for n, t in items]
    blob[f"{kind}/names"] = np.array(json.dumps([r[0] for r in rows]))
    blob[f"{kind}/l2"] = np.array([r[1] for r in rows], dtype=np.float64)
    blob[f"{kind}/count"] = np.array([r[2].size for r in rows], dtype=np.int32)
    blob[f"{kind}/vals"] = np.concatenate([r[2] for r in rows])


TRAIN_CASES = {"b2": (2, 16, 16, 501, "train_stage3_b2_16.npz", 3), "b4": (4, 32, 32, 502, "train_stage3_b4_32.npz", 3)}


def run_train_case(tag):
    """make_golden_train.run_case with the stage-3 weights instead of L1 (its quantities, stored by pack)."""
    crit = reference_losses()
    B, h, w, seed, fname, steps = TRAIN_CASES[tag]
    torch.manual_seed(0)
    model, sd, live_missing = build_cached_mode_model()
    model.train()
    d = {k: torch.from_numpy(v) for k, v in make_train_batch(seed, B, h, w).items()}
    outs = {k: d["out_" + k] for k in ("hat", "dat", "nafnet")}
    feats = {k: d["feat_" + k] for k in ("hat", "dat", "nafnet")}
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    opt = torch.optim.AdamW(model.parameters(), lr=HP["lr"], betas=HP["betas"], weight_decay=HP["weight_decay"], eps=HP["eps"])
    from src.utils.checkpoint_manager import EMAModel
    ema = EMAModel(model, decay=HP["ema_decay"])
    blob = {"meta": np.array(json.dumps({"B": B, "h": h, "w": w, "input_seed": seed, "weight_seed": 1234, "steps": steps, "hp": HP,
                                         "dropout": 0.0, "dead_parameters_not_in_synth": live_missing, "loss_weights": STAGES[3],
                                         "samples": {"full_max": TRAIN_FULL_MAX, "n": TRAIN_NS, "sr_n": SR_NS}}))}
    losses, norms = [], []
    for step in range(steps):
        opt.zero_grad()
        sr = model.forward_with_precomputed(d["lr"], outs, feats).clamp(0, 1)
        loss, comps = combined(crit, STAGES[3], sr, d["hr"])
        loss.backward()
        if step == 0:
            f = sr.detach().reshape(-1).numpy()
            blob["sr/val"] = f[sample_idx("sr", f.size, SR_NS)].astype(np.float32)
            blob["components"] = np.array(json.dumps({k: float(v) for k, v in comps.items()}))
            blob["nograd"] = np.array(json.dumps([n for n, p in named if p.grad is None]))
            pack(blob, "grad", [(n, p.grad) for n, p in named if p.grad is not None])
        gn = torch.nn.utils.clip_grad_norm_(model.parameters(), HP["clip"])
        opt.step()
        ema.update(model)
        losses.append(float(loss))
        norms.append(float(gn))
        print(f"{tag} step {step}: loss {float(loss):.6f}  grad norm {float(gn):.6f}", flush=True)
    blob["losses"] = np.array(losses, dtype=np.float64)
    blob["grad_norms"] = np.array(norms, dtype=np.float64)
    pack(blob, f"param{steps}", [(n, p.data) for n, p in named])
    pack(blob, f"ema{steps}", [(n, ema.shadow[n]) for n, _ in named])
    np.savez_compressed(os.path.join(HERE, fname), **blob)
    print("wrote", fname, os.path.getsize(os.path.join(HERE, fname)) // 1024, "KiB", flush=True)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("FF_THREADS", "8")))
    for a in (sys.argv[1:] or ["losses", "stages"]):
        if a == "losses":
            make_losses()
        elif a == "stages":
            make_stages()
        else:
            run_train_case(a)
