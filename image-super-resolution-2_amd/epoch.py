"""Whole training epochs from a cached-expert directory (isr2_amd/cache.py files), the way the reference runs them:

    train.py:1056-1160   for epoch: warm-up / schedule -> train_epoch_cached -> validate_epoch (EMA weights) -> save latest / best
    train.py:306-383     train_epoch_cached with accumulation_steps = A           -> train_epoch()
    train.py:413-523     validate_epoch, src/utils/metrics.py:291-374             -> validate(), mean_metrics()
    train.py:119-125, :897, :1063-1065, :1105-1107   warm-up + CosineAnnealingWarmRestarts -> lr_for_epoch()
    src/data/cached_dataset.py:147-149, :240-268, :306-315   repeat_factor, paired flips / rotations, shuffle + drop_last -> epoch_plan(), CachedEpoch

The host side of an epoch is file reads and ONE upload per micro-batch: a reader thread fills pinned staging slots (no GPU call
on that thread), the stepping thread copies a slot to the device on a side stream one micro-batch ahead and permutes its eight
tensors with ops.d4_nchw (csrc/augment.hip) -- one launch per tensor per batch.

Two things cannot be bit-compared with the reference, both "parity unpinned (RNG stream)": the attention-dropout masks (train.py
of this package) and the shuffle / augmentation draws, which here come from numpy's counter-based Philox keyed by (seed, epoch) so
that an epoch is reproducible and a resumed run repeats the uninterrupted one.
"""
from __future__ import annotations

import json
import math
import os
import queue
import shutil
import threading
import time
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _lib
from . import cache

T = torch.Tensor
EXPERTS = ("hat", "dat", "nafnet")
SCHEDULE = dict(base_lr=1.5e-4, warmup_epochs=5, warmup_lr=5e-7, T_0=50, T_mult=2, eta_min=5e-8)     # configs/train_config.yaml:102-120


# ======================================================================================================================
# learning rate
def lr_for_epoch(epoch: int, base_lr: float = 1.5e-4, warmup_epochs: int = 5, warmup_lr: float = 5e-7, T_0: int = 50, T_mult: int = 2,
                 eta_min: float = 5e-8) -> float:
    """The learning rate the optimizer holds DURING `epoch` of an uninterrupted reference run (get_current_lr), in closed form.

    It restates the reference's loop, not its YAML: warmup_lr() writes the group's lr only while epoch < warmup_epochs
    (train.py:1063-1065) and CosineAnnealingWarmRestarts.step() runs AFTER an epoch, and only when epoch >= warmup_epochs
    (:1105-1107).  So epoch `warmup_epochs` still trains at the last warm-up value, the cosine starts one epoch later, with
    n = epoch - warmup_epochs scheduler steps behind it, and the first restart lands on epoch warmup_epochs + T_0."""
    epoch = int(epoch)
    if epoch < 0 or T_0 < 1 or T_mult < 1 or warmup_epochs < 0:
        raise _lib.FFError(f"lr_for_epoch: bad arguments epoch={epoch} T_0={T_0} T_mult={T_mult} warmup_epochs={warmup_epochs}")
    if epoch < warmup_epochs:
        return warmup_lr + (base_lr - warmup_lr) * epoch / warmup_epochs                       # train.py:119-125
    if epoch == warmup_epochs:
        # nothing has touched the group since the last warm-up epoch (without warm-up: the scheduler's own initial value)
        return lr_for_epoch(epoch - 1, base_lr, warmup_epochs, warmup_lr, T_0, T_mult, eta_min) if warmup_epochs > 0 else float(base_lr)
    t_cur, t_i = epoch - warmup_epochs, T_0                                                    # scheduler steps taken so far
    while t_cur >= t_i:                                                                        # step(): T_cur -= T_i; T_i *= T_mult
        t_cur -= t_i
        t_i *= T_mult
    return eta_min + (base_lr - eta_min) * (1 + math.cos(math.pi * t_cur / t_i)) / 2


# ======================================================================================================================
# pure host logic: the order of an epoch, its augmentation codes, its accumulation windows, metric averaging
def epoch_plan(n_stems: int, repeat_factor: int, batch_size: int, seed: int, epoch: int, augment: bool = True,
               shuffle: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """-> (idx [nb, batch_size] dataset indices in 0 .. n_stems * repeat_factor, codes [nb, batch_size] D4 codes).
    The dataset has n_stems * repeat_factor entries, entry i reads stem i % n_stems (cached_dataset.py:131-149); the epoch visits
    a shuffled order and drops the incomplete last batch (create_cached_dataloader: shuffle=True, drop_last=True).  Order and codes
    are functions of (seed, epoch) alone -- and a code of (seed, epoch, position in the epoch): code = hflip | vflip << 1 | k << 2,
    uniform over the 16 combinations as the reference's three independent draws are."""
    n = int(n_stems) * int(repeat_factor)
    if n_stems < 1 or repeat_factor < 1 or batch_size < 1:
        raise _lib.FFError(f"epoch_plan: need stems, repeat_factor and batch_size >= 1, got {n_stems}, {repeat_factor}, {batch_size}")
    nb = n // batch_size
    key = [int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFFFFFFFFFF]
    order = np.random.Generator(np.random.Philox(key=key)).permutation(n) if shuffle else np.arange(n)
    codes = np.random.Generator(np.random.Philox(key=key, counter=[0, 0, 0, 1])).integers(0, 16, size=n, dtype=np.int32)
    if not augment:
        codes = np.zeros(n, dtype=np.int32)
    return order[:nb * batch_size].reshape(nb, batch_size).astype(np.int64), codes[:nb * batch_size].reshape(nb, batch_size)


def window_plan(n_micro: int, accumulation_steps: int) -> Tuple[List[dict], int]:
    """The accumulation windows of an epoch of n_micro micro-batches (train.py:306-356): per micro-batch
    {zero_grad, loss_scale, micro_index, step} -- zero_grad before the first micro-batch of a window, step after its last -- and the
    number of trailing micro-batches whose window never completes: they run (BatchNorm statistics advance, their loss is logged)
    but their gradient is discarded by the zero_grad at the top of the next epoch."""
    A = int(accumulation_steps)
    if A < 1 or n_micro < 0:
        raise _lib.FFError(f"window_plan: accumulation_steps {A} must be >= 1 and n_micro {n_micro} >= 0")
    plan = [dict(zero_grad=i % A == 0, loss_scale=1.0 / A, micro_index=i % A, step=(i + 1) % A == 0) for i in range(n_micro)]
    return plan, n_micro % A


def mean_metrics(psnrs: Sequence[float], ssims: Sequence[float]) -> Dict[str, float]:
    """MetricCalculator.update / get_metrics (src/utils/metrics.py:338-374): infinite PSNR values are left out of the PSNR mean only;
    no samples -> {0, 0}."""
    if len(psnrs) != len(ssims):
        raise _lib.FFError("mean_metrics: one PSNR and one SSIM per image")
    if not len(ssims):
        return {"psnr": 0.0, "ssim": 0.0}
    finite = [float(p) for p in psnrs if not math.isinf(p)]
    return {"psnr": float(np.mean(finite)) if finite else 0.0, "ssim": float(np.mean([float(s) for s in ssims]))}


# ======================================================================================================================
# loader
class _Slot:
    """One pinned staging buffer (a whole micro-batch: lr | hr | three expert images | three feature maps | B codes) and its device twin."""

    def __init__(self, layout, n_floats: int, B: int, dev):
        self.host = torch.empty(n_floats + B, dtype=torch.float32, pin_memory=True)
        self.dev = torch.empty(n_floats + B, dtype=torch.float32, device=dev)
        self.views_h = {k: self.host[o:o + int(np.prod(s))].view(s) for k, (o, s) in layout.items()}
        self.views_d = {k: self.dev[o:o + int(np.prod(s))].view(s) for k, (o, s) in layout.items()}
        self.codes_h = self.host[n_floats:].view(torch.int32)
        self.codes_d = self.dev[n_floats:].view(torch.int32)
        self.copied = torch.cuda.Event()                              # the upload of this slot has finished: the host side is free
        self.consumed = None                                          # the permutation kernels that read the device side have been queued
        self.codes = None


class CachedEpoch:
    """Micro-batches of one cache directory, epoch by epoch.

        data = CachedEpoch(cache_dir, batch_size=14, repeat_factor=20, augment=True, seed=0, device="cuda:0")
        for lr, hr, outs, feats in data.batches(epoch): ...           # device tensors, augmented, len(data) of them

    `wait_s` accumulates the time the stepping thread spent waiting for the reader."""

    def __init__(self, cache_dir: str, batch_size: int, repeat_factor: int = 1, augment: bool = True, seed: int = 0, device="cuda:0",
                 prefetch: int = 3, shuffle: bool = True):
        self.dir, self.B, self.repeat, self.augment, self.seed, self.shuffle = cache_dir, int(batch_size), int(repeat_factor), bool(augment), int(seed), shuffle
        self.stems = cache.list_stems(cache_dir)
        if not self.stems:
            raise _lib.FFError(f"{cache_dir}: no cached samples (*{cache.PRIMARY_SUFFIX} + *{cache.REST_SUFFIX})")
        if len(self.stems) * self.repeat < self.B:
            raise _lib.FFError(f"{cache_dir}: {len(self.stems)} samples x repeat {self.repeat} do not fill one batch of {self.B} (drop_last)")
        self.dev = torch.device(device)
        if self.dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.FFError("CachedEpoch needs an MI355X (torch device 'cuda'): the batch is assembled and augmented on the device")
        s = cache.read_sample(cache_dir, self.stems[0])
        shapes = {"lr": tuple(s["lr"].shape), "hr": tuple(s["hr"].shape)}
        shapes.update({"out_" + k: tuple(s["expert_imgs"][k].shape) for k in EXPERTS})
        shapes.update({"feat_" + k: tuple(s["expert_feats"][k].shape) for k in EXPERTS})
        self.layout, n = {}, 0
        for k, shp in shapes.items():
            self.layout[k] = (n, (self.B,) + shp)
            n += self.B * int(np.prod(shp))
        self.n_floats = n
        if self.augment:                                              # refuse before any launch: odd quarter turns need square planes
            from . import ops
            for k, shp in shapes.items():
                ops.d4_check_codes([4], shp[-2], shp[-1])
        self.prefetch = max(2, int(prefetch))
        self._slots = None
        self.wait_s = 0.0

    def __len__(self) -> int:
        return len(self.stems) * self.repeat // self.B

    def plan(self, epoch: int):
        return epoch_plan(len(self.stems), self.repeat, self.B, self.seed, epoch, self.augment, self.shuffle)

    def _fill(self, slot: _Slot, idx, codes):
        for j, i in enumerate(idx):
            s = cache.read_sample(self.dir, self.stems[int(i) % len(self.stems)])
            for k, t in (("lr", s["lr"]), ("hr", s["hr"]), *(("out_" + e, s["expert_imgs"][e]) for e in EXPERTS),
                         *(("feat_" + e, s["expert_feats"][e]) for e in EXPERTS)):
                if tuple(t.shape) != tuple(slot.views_h[k].shape[1:]):
                    raise _lib.FFError(f"cache sample {s['filename']}: {k} has shape {tuple(t.shape)}, the batch holds {tuple(slot.views_h[k].shape[1:])}")
                slot.views_h[k][j].copy_(t)
        slot.codes_h.copy_(torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)))
        slot.codes = [int(c) for c in codes]

    def _reader(self, idx, codes, free: "queue.Queue", ready: "queue.Queue", stop: threading.Event):
        try:
            for b in range(len(idx)):
                slot = free.get()
                if slot is None or stop.is_set():
                    return
                self._fill(slot, idx[b], codes[b])
                ready.put(slot)
            ready.put(None)
        except BaseException as e:                                    # surfaces on the stepping thread
            ready.put(e)

    def batches(self, epoch: int):
        from . import ops
        idx, codes = self.plan(epoch)
        with torch.cuda.device(self.dev):
            if self._slots is None:
                self._slots = [_Slot(self.layout, self.n_floats, self.B, self.dev) for _ in range(self.prefetch)]
                self._copy_stream = torch.cuda.Stream(device=self.dev)
            free, ready, stop = queue.Queue(), queue.Queue(), threading.Event()
            for s in self._slots:
                free.put(s)
            th = threading.Thread(target=self._reader, args=(idx, codes, free, ready, stop), daemon=True)
            th.start()
            main = torch.cuda.current_stream()
            pending: List[_Slot] = []                                 # uploaded, host side not yet known to be free

            def upload():
                """Take the next filled slot and start its copy on the side stream -> the slot, or None at the end of the epoch."""
                for s in [p for p in pending if p.copied.query()]:
                    pending.remove(s)
                    free.put(s)
                t0 = time.perf_counter()
                while True:
                    try:
                        slot = ready.get(timeout=0.0 if pending else None)
                        break
                    except queue.Empty:                               # the reader may be out of slots: hand the oldest one back
                        s = pending.pop(0)
                        s.copied.synchronize()
                        free.put(s)
                self.wait_s += time.perf_counter() - t0
                if isinstance(slot, BaseException):
                    raise slot
                if slot is None:
                    return None
                if slot.consumed is not None:
                    self._copy_stream.wait_event(slot.consumed)       # the device twin is still being read by the previous round's kernels
                with torch.cuda.stream(self._copy_stream):
                    slot.dev.copy_(slot.host, non_blocking=True)      # ONE upload per micro-batch
                    slot.copied.record(self._copy_stream)
                pending.append(slot)
                return slot

            try:
                nxt = upload()
                while nxt is not None:
                    cur, nxt = nxt, None
                    main.wait_event(cur.copied)
                    out = {k: ops.d4_nchw(v, cur.codes, codes_dev=cur.codes_d) for k, v in cur.views_d.items()}   # 8 launches
                    cur.consumed = torch.cuda.Event()
                    cur.consumed.record(main)
                    nxt = upload()                                    # one micro-batch ahead of the step about to be queued
                    yield (out["lr"], out["hr"], {e: out["out_" + e] for e in EXPERTS}, {e: out["feat_" + e] for e in EXPERTS})
            finally:
                stop.set()
                free.put(None)
                for s in pending:
                    s.copied.synchronize()
                th.join(timeout=60)


def read_samples(cache_dir: str) -> Iterable[dict]:
    """Every sample of a (validation) cache directory, as cache.read_sample returns it."""
    for stem in cache.list_stems(cache_dir):
        yield cache.read_sample(cache_dir, stem)


# ======================================================================================================================
# epoch, validation, driver
def train_epoch(trainer, epoch_data, epoch: int, accumulation_steps: int = 1, lr_now: Optional[float] = None, grad_hook=None) -> dict:
    """train_epoch_cached (train.py:262-383): -> {'loss', 'stage', component means..., 'lr', 'micro_batches', 'optimizer_steps', 'discarded'}.
    epoch_data: a CachedEpoch, or any iterable of (lr, hr, outs, feats) micro-batches for this epoch."""
    stage = trainer.set_epoch(epoch)
    lr_now = lr_for_epoch(epoch, base_lr=trainer.hp["lr"]) if lr_now is None else float(lr_now)
    it = epoch_data.batches(epoch) if hasattr(epoch_data, "batches") else iter(epoch_data)
    A = int(accumulation_steps)
    window_plan(0, A)                                                 # argument check
    trainer.discard_window()                                          # optimizer.zero_grad() at the top of the epoch (train.py:306)
    losses, comps, n, steps = [], {}, 0, 0
    for lr, hr, outs, feats in it:
        w = window_plan(n + 1, A)[0][n]
        _, loss = trainer.forward_backward(lr, hr, outs, feats, zero_grad=w["zero_grad"], loss_scale=w["loss_scale"], micro_index=w["micro_index"])
        losses.append(loss.clone())
        if not trainer._default_loss:
            comps[n] = trainer.loss_values[:len(trainer.active_losses)].clone()
        if w["step"]:
            if grad_hook is not None:
                grad_hook(trainer.G)
            trainer.optimizer_step(lr_now)
            steps += 1
        n += 1
    discarded = n % A
    if discarded:
        trainer.discard_window()
    res = {"loss": 0.0, "stage": stage, "lr": lr_now, "micro_batches": n, "optimizer_steps": steps, "discarded": discarded}
    if n:
        lv = torch.cat(losses).double().cpu()                        # one read-back per epoch
        res["loss"] = float(lv.mean())
        res["micro_losses"] = [float(v) for v in lv]
        if trainer._default_loss:
            res["l1"] = res["loss"]
        else:
            cv = torch.stack([comps[i] for i in range(n)]).double().mean(0).cpu().tolist()
            res.update({k: float(v) for (k, _), v in zip(trainer.active_losses, cv)})
    return res


@torch.no_grad()
def validate(trainer, samples: Iterable[dict], use_ema: bool = True, crop_border: int = 4, test_y_channel: bool = True,
             return_sr: bool = False, batch: int = 1) -> dict:
    """validate_epoch (train.py:413-523) in cached mode -> {'psnr', 'ssim'}: the eval-mode forward_with_precomputed of a FusionHIP
    built from the EMA shadow (use_ema) or the parameters, with the trainer's current BatchNorm buffers, one image per call;
    clamp(0, 1); per-image PSNR / SSIM on the device (isr2_amd.metrics), averaged as MetricCalculator does.  The trainer's own
    state is only read.  samples: dicts as cache.read_sample returns them (lr [3,h,w], hr, expert_imgs, expert_feats).
    batch > 1: up to `batch` consecutive samples of equal shapes (and the same feature keys) go through ONE FusionHIP.forward, one launch
    per op for the group; a sample that differs starts a new group.  PSNR / SSIM stay per image, and `sr` / `per_image` are bit-equal
    to batch = 1 (the default: one forward per sample, launch for launch what it always was)."""
    from . import metrics, ops
    from . import autograd as ag
    from .fusion import FusionHIP
    sd = trainer.state_dict()                                         # parameters + BatchNorm buffers + fixed tensors, host copies
    if use_ema:
        sd.update(trainer.ema_shadow())
    old_mode = ops.gemm_mode()
    if trainer.gemm is not None:
        ops.set_gemm_mode(trainer.gemm)
    psnrs, ssims, srs = [], [], []
    try:
        with torch.cuda.device(trainer.dev):
            model = FusionHIP(sd, trainer.dev)
            to4 = lambda t: (t.unsqueeze(0) if t.dim() == 3 else t).to(trainer.dev, torch.float32).contiguous()      # noqa: E731

            def load(s):
                lr, hr = to4(s["lr"]), to4(s["hr"])
                if lr.shape[0] != 1:
                    raise _lib.FFError("validate: one image per sample")
                feats = s.get("expert_feats")
                return lr, hr, {k: to4(v) for k, v in s["expert_imgs"].items()}, ({k: to4(v) for k, v in feats.items()} if feats else None)

            def shapes(g):
                return (tuple(g[0].shape), tuple(g[1].shape), tuple(sorted((k, tuple(v.shape)) for k, v in g[2].items())),
                        tuple(sorted((k, tuple(v.shape)) for k, v in g[3].items())) if g[3] else None)

            def run(group):
                if len(group) == 1:
                    lr, hr, ex, feats = group[0]
                else:                                                 # consecutive samples of one shape: one forward for all of them
                    cat = lambda ts: torch.cat(list(ts))              # noqa: E731
                    lr, hr = cat(g[0] for g in group), cat(g[1] for g in group)
                    ex = {k: cat(g[2][k] for g in group) for k in group[0][2]}
                    feats = {k: cat(g[3][k] for g in group) for k in group[0][3]} if group[0][3] else None
                sr = model.forward(lr, ex, feats=feats)
                sr = ag.k_unary("clamp01", sr)                        # sr.clamp(0, 1), train.py:482
                hr = ag.k_unary("clamp01", hr)                        # MetricCalculator.update, metrics.py:333-334
                for b in range(len(group)):
                    psnrs.append(metrics.calculate_psnr(sr[b], hr[b], crop_border, test_y_channel))
                    ssims.append(metrics.calculate_ssim(sr[b], hr[b], crop_border, test_y_channel))
                    if return_sr:
                        srs.append(sr[b].cpu())

            group = []
            for s in samples:
                g = load(s)
                if group and (len(group) >= max(1, int(batch)) or shapes(g) != shapes(group[0])):
                    run(group)
                    group = []
                group.append(g)
            if group:
                run(group)
    finally:
        ops.set_gemm_mode(old_mode)
    res = mean_metrics(psnrs, ssims)
    if return_sr:
        res.update(sr=srs, per_image=list(zip(psnrs, ssims)))
    return res


def fit(trainer, train_data, val_samples, out_dir: str, epochs: int, start_epoch: int = 0, accumulation_steps: int = 2, validate_every: int = 1,
        best_psnr: float = float("-inf"), schedule: Optional[dict] = None, log=print) -> dict:
    """The reference's epoch loop (train.py:1056-1160): per epoch train -> validate with EMA weights (every `validate_every` epochs and
    the last one) -> latest.pth, copied to best.pth on a new best PSNR.  One JSON line per epoch through `log`.
    val_samples: a callable returning an iterable of samples (called per validation), or a list."""
    os.makedirs(out_dir, exist_ok=True)
    latest, best = os.path.join(out_dir, "latest.pth"), os.path.join(out_dir, "best.pth")
    sched = dict(SCHEDULE, base_lr=trainer.hp["lr"], **(schedule or {}))
    last = {}
    for epoch in range(int(start_epoch), int(epochs)):
        t0 = time.perf_counter()
        lr_now = lr_for_epoch(epoch, **sched)
        if hasattr(train_data, "wait_s"):
            train_data.wait_s = 0.0
        tm = train_epoch(trainer, train_data, epoch, accumulation_steps, lr_now)
        tm.pop("micro_losses", None)
        torch.cuda.synchronize(trainer.dev)
        t1 = time.perf_counter()
        row = dict(epoch=epoch, **tm, train_s=t1 - t0, data_wait_s=getattr(train_data, "wait_s", 0.0))
        metrics_now = {}
        if (epoch + 1) % max(1, int(validate_every)) == 0 or epoch == int(epochs) - 1:
            metrics_now = validate(trainer, val_samples() if callable(val_samples) else val_samples, use_ema=True)
            row.update(metrics_now, val_s=time.perf_counter() - t1)
        trainer.save_checkpoint(latest, epoch=epoch, metrics=dict(metrics_now, loss=tm["loss"], best_psnr=max(best_psnr, metrics_now.get("psnr", best_psnr))),
                                lr_now=lr_now)
        if metrics_now and metrics_now["psnr"] > best_psnr:
            best_psnr = metrics_now["psnr"]
            shutil.copyfile(latest, best)
            row["best"] = True
        log(json.dumps(row))
        last = row
    return dict(last, best_psnr=best_psnr)
