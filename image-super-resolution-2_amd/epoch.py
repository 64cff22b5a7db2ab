"""Whole training epochs, the way the reference runs them -- from a cached-expert directory (isr2_amd/cache.py files):

    train.py:1056-1160   for epoch: warm-up / schedule -> train_epoch_cached -> validate_epoch (EMA weights) -> save latest / best
    train.py:306-383     train_epoch_cached with accumulation_steps = A           -> train_epoch()
    train.py:413-523     validate_epoch, src/utils/metrics.py:291-374             -> validate(), mean_metrics()
    train.py:119-125, :897, :1063-1065, :1105-1107   warm-up + CosineAnnealingWarmRestarts -> lr_for_epoch()
    src/data/cached_dataset.py:147-149, :240-268, :306-315   repeat_factor, paired flips / rotations, shuffle + drop_last -> epoch_plan(), CachedEpoch

The host side of an epoch is file reads and ONE upload per micro-batch: a reader thread fills pinned staging slots (no GPU call
on that thread: staging.ReadAhead, which the pools and the cache builder use too), the stepping thread copies a slot to the device
on a side stream one micro-batch ahead and permutes its eight tensors with ops.d4_nchw (csrc/augment.hip) -- one launch per tensor per batch.  Opt-in, ResidentCache / ResidentEpoch read every
sample ONCE into one device buffer and assemble each augmented micro-batch with one launch (csrc/gather_batch.hip), the same bits.

Two things cannot be bit-compared with the reference, both "parity unpinned (RNG stream)": the attention-dropout masks (train.py
of this package) and the shuffle / augmentation draws, which here come from numpy's counter-based Philox keyed by (seed, epoch) so
that an epoch is reproducible and a resumed run repeats the uninterrupted one.

-- or from image folders with the three frozen experts run on every micro-batch (train.py:130-250 train_epoch, what the shipped
configuration selects: dataset.train.cache_data false, repeat_factor 6):

    src/data/dataset.py:236-296, :562-565; augmentations.py:77-79, :128-135, :169-171   -> live_plan(), ImagePool, LiveEpoch
    train.py:413-523 on centre patches                                                     -> live_val_samples()
    train.py:413-523 on ValidationDataset's resized whole images (dataset.py:473-506)      -> live_val_images(), val_resized_shape()

The images are decoded once into one device buffer; a micro-batch is one sampler launch (csrc/sample_batch.hip: crop, u8 -> fp32
and the paired D4 symmetry) and one replay of the captured expert graph, with nothing read from disk.  Its crop and augmentation
draws are a third "parity unpinned (RNG stream)".  LiveEpoch(color_jitter=...) adds the reference's paired colour jitter
(augmentations.py:207-264 -> live_jitter_plan(), csrc/color_jitter.hip) between the two: its draws are one more unpinned RNG stream,
and its 8-bit HSV step restates OpenCV's published definition without an OpenCV binary to compare with: "parity unpinned (OpenCV absent)".
"""
from __future__ import annotations

import json
import math
import os
import shutil
import time
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as _lib
from . import cache
from .cache import EXPERTS, FIELDS                                    # the eight tensors of a cached sample, in CachedEpoch.layout's order
from .staging import ReadAhead

T = torch.Tensor
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
        shapes = {k: tuple(t.shape) for k, t in cache.sample_fields(cache.read_sample(cache_dir, self.stems[0])).items()}
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
            for k, t in cache.sample_fields(s).items():
                if tuple(t.shape) != tuple(slot.views_h[k].shape[1:]):
                    raise _lib.FFError(f"cache sample {s['filename']}: {k} has shape {tuple(t.shape)}, the batch holds {tuple(slot.views_h[k].shape[1:])}")
                slot.views_h[k][j].copy_(t)
        slot.codes_h.copy_(torch.from_numpy(np.ascontiguousarray(codes, dtype=np.int32)))
        slot.codes = [int(c) for c in codes]

    def batches(self, epoch: int):
        from . import ops
        idx, codes = self.plan(epoch)
        with torch.cuda.device(self.dev):
            if self._slots is None:
                self._slots = [_Slot(self.layout, self.n_floats, self.B, self.dev) for _ in range(self.prefetch)]
                self._copy_stream = torch.cuda.Stream(device=self.dev)
            main = torch.cuda.current_stream()
            slots = iter(self._slots)
            reads = ReadAhead(len(idx), lambda b, slot: self._fill(slot, idx[b], codes[b]), lambda: next(slots), n_slots=self.prefetch,
                              name="ff-epoch-reader")                 # items are micro-batches: one reader, so they arrive in order
            filled = iter(reads)

            def upload():
                """Take the next filled slot and start its copy on the side stream -> the slot, or None at the end of the epoch."""
                slot = next(filled, (None, None, None))[1]
                if slot is None:
                    return None
                if slot.consumed is not None:
                    self._copy_stream.wait_event(slot.consumed)       # the device twin is still being read by the previous round's kernels
                with torch.cuda.stream(self._copy_stream):
                    slot.dev.copy_(slot.host, non_blocking=True)      # ONE upload per micro-batch
                    slot.copied.record(self._copy_stream)
                reads.release(slot, slot.copied)                      # the host side is free once the upload has finished
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
                    yield cache.fields_batch(out)
            finally:
                reads.close()                                         # an abandoned epoch too: the reader ended, the uploads finished
                self.wait_s += reads.wait_s


def read_samples(cache_dir: str) -> Iterable[dict]:
    """Every sample of a (validation) cache directory, as cache.read_sample returns it."""
    for stem in cache.list_stems(cache_dir):
        yield cache.read_sample(cache_dir, stem)


# ======================================================================================================================
# the cache resident on the device: every sample loaded ONCE, a micro-batch assembled by one launch (csrc/gather_batch.hip)
RESIDENT_ALIGN = 64                                                   # floats: every field starts on a 256-byte boundary


def resident_layout(shapes: Sequence[Tuple[int, ...]], n: int) -> Tuple[np.ndarray, int]:
    """The field-major layout of n samples: shapes = one (C, H, W) per field -> (offsets int64 [F] in floats, total floats).  Field f
    is a contiguous [n, C, H, W] array at offsets[f]; every field starts on a multiple of 64 floats, so a field whose W is a multiple
    of 4 takes the kernel's 16-byte form whatever came before it.  total = the end of the last field (no padding after it)."""
    n = int(n)
    if n < 1 or not len(shapes):
        raise _lib.FFError(f"resident_layout: need fields and n >= 1, got {len(shapes)} fields and n = {n}")
    offs, end = np.zeros(len(shapes), dtype=np.int64), 0
    for f, shp in enumerate(shapes):
        if len(shp) != 3 or min(int(v) for v in shp) < 1:
            raise _lib.FFError(f"resident_layout: field {f} has shape {tuple(shp)}, expected (C, H, W) >= 1")
        offs[f] = -(-end // RESIDENT_ALIGN) * RESIDENT_ALIGN
        end = int(offs[f]) + n * int(shp[0]) * int(shp[1]) * int(shp[2])
    return offs, end


class ResidentCache:
    """Every sample of a cache directory, loaded once and resident on the device as ONE field-major fp32 buffer.

        pool = ResidentCache(cache_dir, device="cuda:0", readers=8, max_bytes=200 << 30)
        pool.buf [total_floats] fp32, pool.shapes {field: (C, H, W)}, pool.offsets int64 [8], pool.stems, pool.load_s

    The eight field shapes come from the first sample (as CachedEpoch takes them) and the pool is laid out from them by
    resident_layout; more than max_bytes is an error naming the bytes needed, raised before anything is allocated -- there is no
    second route.  Then `readers` host threads (at most 16) run cache.read_sample into pinned one-sample slots and make no GPU call;
    the calling thread uploads each sample into its eight places (staging.ReadAhead, as ImagePool does).  A sample whose shapes
    differ from the first one's is an error naming the file.  `load_s`: seconds the loading took."""

    def __init__(self, cache_dir: str, device="cuda:0", readers: int = 8, max_bytes: int = 200 << 30):
        self.dir, self.dev = cache_dir, torch.device(device)
        if int(readers) < 1:
            raise _lib.FFError(f"ResidentCache: readers must be >= 1, got {readers}")
        self.stems = cache.list_stems(cache_dir)
        if not self.stems:
            raise _lib.FFError(f"{cache_dir}: no cached samples (*{cache.PRIMARY_SUFFIX} + *{cache.REST_SUFFIX})")
        t0 = time.perf_counter()
        first = cache.sample_fields(cache.read_sample(cache_dir, self.stems[0]))
        self.shapes = {k: tuple(int(v) for v in first[k].shape) for k in FIELDS}
        n = len(self.stems)
        self.offsets, self.total_floats = resident_layout([self.shapes[k] for k in FIELDS], n)
        self.total_bytes = 4 * self.total_floats
        if self.total_bytes > int(max_bytes):
            raise _lib.FFError(f"ResidentCache: {n} samples need {self.total_bytes} bytes on the device, max_bytes allows {int(max_bytes)}")
        if self.dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.FFError("ResidentCache needs an MI355X (torch device 'cuda'): the samples live on the device")
        self.readers = max(1, min(16, int(readers)))
        with torch.cuda.device(self.dev):
            self.buf = torch.empty(self.total_floats, dtype=torch.float32, device=self.dev)
            self._fill()
        self.load_s = time.perf_counter() - t0

    def _fill(self):
        sizes = [int(np.prod(self.shapes[k])) for k in FIELDS]
        soffs, slot_floats = resident_layout([self.shapes[k] for k in FIELDS], 1)      # one sample: the slot's own layout

        def read(i, slot):
            s = cache.read_sample(self.dir, self.stems[i])
            for k, so, t in zip(FIELDS, soffs, cache.sample_fields(s).values()):
                if tuple(t.shape) != self.shapes[k]:
                    raise _lib.FFError(f"{os.path.join(self.dir, self.stems[i] + cache.PRIMARY_SUFFIX)}: {k} has shape {tuple(t.shape)}, the pool "
                                       f"holds {self.shapes[k]} (the shapes of {self.stems[0]})")
                slot[int(so):int(so) + t.numel()].view(t.shape).copy_(t)

        def upload(i, slot):
            for po, so, sz in zip(self.offsets, soffs, sizes):
                self.buf[int(po) + i * sz:int(po) + (i + 1) * sz].copy_(slot[int(so):int(so) + sz], non_blocking=True)

        with ReadAhead(len(self.stems), read, lambda: torch.empty(slot_floats, dtype=torch.float32, pin_memory=True), self.readers,
                       name="ff-cache-reader") as reads:
            for i, slot, _ in reads:                                  # arrival order: every sample has its own place in the pool
                upload(i, slot)
                reads.release(slot, cache.recorded_event())
        torch.cuda.synchronize(self.dev)

    def __len__(self) -> int:
        return len(self.stems)

    def field(self, name: str) -> T:
        """[n, C, H, W]: the view of one field inside the pool."""
        f = FIELDS.index(name)
        C, H, W = self.shapes[name]
        return self.buf[int(self.offsets[f]):int(self.offsets[f]) + len(self) * C * H * W].view(len(self), C, H, W)

    def sample(self, i: int) -> dict:
        """Sample i in cache.read_sample's shape; its tensors are views of the pool."""
        return cache.fields_sample({k: self.field(k)[i] for k in FIELDS}, self.stems[i])

    def samples(self) -> Iterable[dict]:
        """Every sample as read_samples yields them, from the pool: validate() takes them unchanged (its .to(device) is a no-op)."""
        for i in range(len(self)):
            yield self.sample(i)


class ResidentEpoch:
    """Micro-batches of a ResidentCache, epoch by epoch; interchangeable with CachedEpoch in train_epoch and fit, and bit-equal to it.

        data = ResidentEpoch(pool, batch_size=14, repeat_factor=20, augment=True, seed=0)
        for lr, hr, outs, feats in data.batches(epoch): ...           # device tensors, augmented, len(data) of them

    plan() is epoch_plan itself: order and codes are CachedEpoch's for the same (seed, epoch).  An epoch uploads its descriptor table
    (int32 [nb, B, 2] = {sample index, d4 code}) once; a micro-batch is then one fresh flat buffer from the caching allocator and ONE
    ops.gather_d4_fields launch on the current stream, and the eight yielded tensors are views of that buffer.  No thread, no side
    stream, no copy and nothing read from disk during an epoch: `wait_s` stays 0."""

    def __init__(self, pool: ResidentCache, batch_size: int, repeat_factor: int = 1, augment: bool = True, seed: int = 0, shuffle: bool = True):
        self.pool, self.B, self.repeat, self.augment, self.seed, self.shuffle = pool, int(batch_size), int(repeat_factor), bool(augment), int(seed), shuffle
        self.stems, self.dev = pool.stems, pool.dev
        if self.B < 1 or self.repeat < 1:
            raise _lib.FFError(f"ResidentEpoch: batch_size and repeat_factor must be >= 1, got {batch_size}, {repeat_factor}")
        if len(self.stems) * self.repeat < self.B:
            raise _lib.FFError(f"{pool.dir}: {len(self.stems)} samples x repeat {self.repeat} do not fill one batch of {self.B} (drop_last)")
        if self.augment:                                              # refuse before any launch: odd quarter turns need square planes
            from . import ops
            for k in FIELDS:
                ops.d4_check_codes([4], pool.shapes[k][-2], pool.shapes[k][-1])
        shapes = [pool.shapes[k] for k in FIELDS]
        self.out_offsets, self.out_floats = resident_layout(shapes, self.B)
        self.fields = np.array([[int(po), int(oo), *shp] for po, oo, shp in zip(pool.offsets, self.out_offsets, shapes)], dtype=np.int64)
        self.wait_s = 0.0

    def __len__(self) -> int:
        return len(self.stems) * self.repeat // self.B

    def plan(self, epoch: int):
        return epoch_plan(len(self.stems), self.repeat, self.B, self.seed, epoch, self.augment, self.shuffle)

    def descriptors(self, epoch: int) -> np.ndarray:
        """The epoch's gather table, int32 [nb, B, 2] = {sample index, d4 code} (ops.gather_d4_fields)."""
        idx, codes = self.plan(epoch)
        return np.ascontiguousarray(np.stack((idx % len(self.stems), codes), axis=-1).astype(np.int32))

    def batches(self, epoch: int):
        from . import ops
        desc = self.descriptors(epoch)
        with torch.cuda.device(self.dev):
            desc_dev = torch.from_numpy(desc).to(self.dev)            # ONE upload per epoch
            for b in range(desc.shape[0]):
                flat = torch.empty(self.out_floats, dtype=torch.float32, device=self.dev)
                yield cache.fields_batch(dict(zip(FIELDS, ops.gather_d4_fields(self.pool.buf, len(self.stems), self.fields, desc_dev[b], flat,
                                                                                desc_host=desc[b]))))


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
        best_psnr: float = float("-inf"), schedule: Optional[dict] = None, log=print, validate_start: int = 0) -> dict:
    """The reference's epoch loop (train.py:1056-1160): per epoch train -> validate with EMA weights (every `validate_every` epochs and
    the last one) -> latest.pth, copied to best.pth on a new best PSNR.  One JSON line per epoch through `log`.
    val_samples: a callable returning an iterable of samples (called per validation), or a list.
    validate_start: no validation in epochs before it (the reference's validation.validate_start, train.py:1116-1119), the last epoch
    excepted.  The every-N rule here is (epoch + 1) % N == 0; the reference tests epoch % N == 0."""
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
        if (epoch >= int(validate_start) and (epoch + 1) % max(1, int(validate_every)) == 0) or epoch == int(epochs) - 1:
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


# ======================================================================================================================
# live experts: micro-batches cut from image folders, the three frozen experts run on every batch (the reference's train_epoch,
# train.py:130-250, which configs/train_config.yaml selects with dataset.train.cache_data: false and repeat_factor: 6)
def pool_members(sizes: Sequence[Tuple[int, int]], patch: int) -> Tuple[List[int], int]:
    """-> (positions in `sizes` of the LR images (h, w) that hold a patch x patch crop, number of images left out).  The reference
    resizes smaller images with OpenCV (dataset.py:262-280); that is not reproduced, they are skipped and counted as in crop_plan."""
    p = int(patch)
    if p < 1:
        raise _lib.FFError(f"pool_members: patch {p} must be >= 1")
    keep = [i for i, (h, w) in enumerate(sizes) if int(h) >= p and int(w) >= p]
    return keep, len(sizes) - len(keep)


def pool_layout(sizes: Sequence[Tuple[int, int]]) -> Tuple[np.ndarray, int]:
    """The packed layout of an ImagePool: sizes = LR (h, w) per image -> (offsets int64 [n, 2] = byte offsets of the LR image
    [h][w][3] and of its HR partner [4h][4w][3], total bytes).  uint8 HWC, back to back in list order, LR before HR, no padding."""
    offs, n = np.zeros((len(sizes), 2), dtype=np.int64), 0
    for i, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise _lib.FFError(f"pool_layout: image {i} has size {h}x{w}")
        offs[i] = (n, n + 3 * h * w)
        n += 51 * h * w                                               # 3 h w + 3 (4h) (4w)
    return offs, n


def live_plan(sizes: Sequence[Tuple[int, int]], repeat_factor: int, batch_size: int, patch: int, seed: int, epoch: int, augment: bool = True,
              shuffle: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """-> (idx, top, left, codes), each [nb, batch_size]: dataset indices in 0 .. n_images * repeat_factor (entry i reads image
    i % n_images, dataset.py:236-249), the LR patch origin and the D4 code of every sample of the epoch.  Shuffled order, incomplete
    last batch dropped (dataset.py:562-565).  sizes = LR (h, w) per image, all >= patch.  The draws restate the reference's
    augmentation: top uniform in [0, h - p], left uniform in [0, w - p] (augmentations.py:77-79), hflip and vflip with p = 0.5 each
    (:128-135), and a rotation with p = 0.5 whose k is uniform in {1, 2, 3} (:169-171) -- k = 0 half of the time, NOT the uniform k of
    the cached mode.  augment=False: code 0 at the centre position ((h - p) // 2, (w - p) // 2) (dataset.py:282-296).
    Everything is a function of (seed, epoch) through numpy's counter-based Philox -- a draw belongs to a position in the epoch --
    so a resumed run repeats the uninterrupted one; the reference's own streams: parity unpinned (RNG stream)."""
    n_img, p = len(sizes), int(patch)
    if n_img < 1 or repeat_factor < 1 or batch_size < 1 or p < 1:
        raise _lib.FFError(f"live_plan: need images, repeat_factor, batch_size and patch >= 1, got {n_img}, {repeat_factor}, {batch_size}, {p}")
    hw = np.asarray(sizes, dtype=np.int64).reshape(n_img, 2)
    if (hw < p).any():
        raise _lib.FFError(f"live_plan: image {int(np.argmax((hw < p).any(axis=1)))} is smaller than the {p}x{p} patch")
    n = n_img * int(repeat_factor)
    nb = n // int(batch_size)
    m = nb * int(batch_size)
    key = [int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFFFFFFFFFF]
    gen = lambda c: np.random.Generator(np.random.Philox(key=key, counter=[0, 0, 0, c]))     # noqa: E731 -- one stream per quantity
    order = (gen(0).permutation(n) if shuffle else np.arange(n))[:m].astype(np.int64)
    room = hw[order % n_img] - p                                      # [m, 2]: the largest top / left of each sample's image
    if augment:
        top = gen(1).integers(0, room[:, 0] + 1, dtype=np.int64)
        left = gen(2).integers(0, room[:, 1] + 1, dtype=np.int64)
        flips = gen(3).integers(0, 4, size=m, dtype=np.int64)         # bit 0 hflip, bit 1 vflip: two independent fair draws
        turn = gen(4).integers(0, 2, size=m, dtype=np.int64)          # rotate at all?
        k = np.where(turn == 1, gen(5).integers(1, 4, size=m, dtype=np.int64), 0)
        codes = (flips | (k << 2)).astype(np.int32)
    else:
        top, left, codes = room[:, 0] // 2, room[:, 1] // 2, np.zeros(m, dtype=np.int32)
    shp = (nb, int(batch_size))
    return order.reshape(shp), top.reshape(shp), left.reshape(shp), codes.reshape(shp)


JITTER_DEFAULTS = dict(prob=0.5, brightness=0.2, contrast=0.2, saturation=0.2)   # ColorJitter's and SRTrainAugmentation's class defaults


def live_jitter_plan(nb: int, batch_size: int, seed: int, epoch: int, prob: float = 0.5, brightness: float = 0.2, contrast: float = 0.2,
                     saturation: float = 0.2) -> np.ndarray:
    """-> fp32 [nb, batch_size, 4] = {apply, bf, cf, sf}: the colour-jitter table of an epoch (ops.color_jitter_pairs), one row per sample
    of live_plan's epoch.  The reference (augmentations.py:222-228): apply = random() < prob; each factor = 1 + uniform(-r, r), shared by
    the LR and the HR patch.  The training set is built without jitter arguments (dataset.py:111-119), so the class defaults hold --
    prob 0.5 and 0.2 for the three ranges -- not the YAML's values, which are never read.  Drawn in fp64 and rounded to fp32; a row keeps
    its drawn factors when apply is 0.  live_plan's Philox key with counters 6..9 (apply, brightness, contrast, saturation): live_plan's
    own streams 0..5 are untouched, and the table is a function of (seed, epoch) only, so a resumed run repeats the uninterrupted one.
    The reference's `random` stream: parity unpinned (RNG stream)."""
    nb, B = int(nb), int(batch_size)
    rng = (float(brightness), float(contrast), float(saturation))
    if nb < 0 or B < 1 or not 0.0 <= float(prob) <= 1.0 or not all(0.0 <= r < 1.0 for r in rng):
        raise _lib.FFError(f"live_jitter_plan: need nb >= 0, batch_size >= 1, prob in [0, 1] and ranges in [0, 1), got {nb}, {B}, {prob}, {rng}")
    m = nb * B
    key = [int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch) & 0xFFFFFFFFFFFFFFFF]
    gen = lambda c: np.random.Generator(np.random.Philox(key=key, counter=[0, 0, 0, c]))     # noqa: E731 -- one stream per quantity
    t = np.empty((m, 4), dtype=np.float32)
    t[:, 0] = gen(6).random(m) < float(prob)
    for j, r in enumerate(rng):
        t[:, 1 + j] = (1.0 + gen(7 + j).uniform(-r, r, size=m)).astype(np.float32)
    return t.reshape(nb, B, 4)


class ImagePool:
    """Every image pair of a folder (or two), decoded once and resident on the device as ONE packed uint8 buffer.

        pool = ImagePool(hr_dir, lr_dir=None, patch=64, device="cuda:0", readers=8, max_bytes=64 << 30)
        pool.buf [total_bytes] uint8, pool.sizes [(h, w)] LR sizes, pool.offsets int64 [n, 2], pool.stems, pool.skipped

    Pairing and order are cache.list_pairs', as in cache.build_from_folders: matched by stem, sorted, image index = position in that order (among the
    images kept).  Pass 1 reads the sizes from the headers, leaves out (and counts) images smaller than the patch, lays the pool out
    (pool_layout) and allocates it; more than max_bytes is an error -- there is no second route.  Pass 2: `readers` host threads
    (at most 16) decode into pinned uint8 slots and make no GPU call; the calling thread uploads each image into its place.
    With lr_dir an HR image that is not exactly 4x its LR partner is an error naming the file (skip_mismatched: left out and counted in
    `skipped` instead: live_val_images).  Without it HR is cropped top-left to
    multiples of 4 and LR = f32_to_u8_image(resize_aa(u8_to_f32_image(hr))) on the device, as build_from_folders makes it.
    A reader's exception ends construction and is re-raised."""

    def __init__(self, hr_dir: str, lr_dir: Optional[str] = None, patch: int = 64, device="cuda:0", readers: int = 8, max_bytes: int = 64 << 30,
                 skip_mismatched: bool = False):
        from PIL import Image
        self.patch, self.dev = int(patch), torch.device(device)
        if self.patch < 1 or int(readers) < 1:
            raise _lib.FFError(f"ImagePool: patch and readers must be >= 1, got {patch}, {readers}")
        if self.dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.FFError("ImagePool needs an MI355X (torch device 'cuda'): the images live on the device")
        items, sizes, paired = cache.list_pairs(hr_dir, lr_dir), [], []
        for stem, hr_path, lr_path in items:                          # pass 1: headers only
            W, H = Image.open(hr_path).size
            if lr_path is None:
                h, w = H // 4, W // 4
            else:
                w, h = Image.open(lr_path).size
                if (H, W) != (4 * h, 4 * w):
                    if skip_mismatched:
                        continue
                    raise _lib.FFError(f"{hr_path}: HR is {H}x{W}, not exactly 4x its LR {lr_path} ({h}x{w})")
            sizes.append((h, w))
            paired.append((stem, hr_path, lr_path))
        mismatched, items = len(items) - len(paired), paired
        keep, self.skipped = pool_members(sizes, self.patch)
        self.skipped += mismatched
        if not keep:
            raise _lib.FFError(f"{hr_dir}: no image holds a {self.patch}x{self.patch} LR patch ({self.skipped} skipped)")
        self.stems = [items[i][0] for i in keep]
        self.sizes = [sizes[i] for i in keep]
        self.offsets, self.total_bytes = pool_layout(self.sizes)
        if self.total_bytes > int(max_bytes):
            raise _lib.FFError(f"ImagePool: {len(keep)} images need {self.total_bytes} bytes on the device, max_bytes allows {int(max_bytes)}")
        with torch.cuda.device(self.dev):
            self.buf = torch.empty(self.total_bytes, dtype=torch.uint8, device=self.dev)
            self._fill([items[i] for i in keep], lr_dir is None, max(1, min(16, int(readers))))

    def _fill(self, items, hr_only: bool, n_readers: int):
        from . import ops
        from PIL import Image
        slot_bytes = max(51 * h * w for h, w in self.sizes)

        def read(i, slot):
            (h, w), (_, hr_path, lr_path) = self.sizes[i], items[i]
            hr = np.asarray(Image.open(hr_path).convert("RGB"), dtype=np.uint8)[:4 * h, :4 * w]
            if hr.shape != (4 * h, 4 * w, 3):
                raise _lib.FFError(f"{hr_path}: decoded to {hr.shape[0]}x{hr.shape[1]}, its header said {4 * h}x{4 * w} or more")
            slot[3 * h * w:51 * h * w].view(4 * h, 4 * w, 3).numpy()[...] = hr
            if lr_path is not None:
                lr = np.asarray(Image.open(lr_path).convert("RGB"), dtype=np.uint8)
                if lr.shape != (h, w, 3):
                    raise _lib.FFError(f"{lr_path}: decoded to {lr.shape[0]}x{lr.shape[1]}, its header said {h}x{w}")
                slot[:3 * h * w].view(h, w, 3).numpy()[...] = lr

        def upload(i, slot):
            (h, w), (lo, ho) = self.sizes[i], (int(v) for v in self.offsets[i])
            if hr_only:                                               # the LR image is made here, from the uploaded HR image
                hr_u8 = slot[3 * h * w:51 * h * w].view(4 * h, 4 * w, 3).to(self.dev, non_blocking=True)
                self.buf[ho:ho + 48 * h * w].copy_(hr_u8.view(-1))
                lr_u8 = ops.f32_to_u8_image(ops.resize_aa(ops.u8_to_f32_image(hr_u8), (h, w)))
                self.buf[lo:lo + 3 * h * w].copy_(lr_u8.view(-1))
            else:                                                     # LR and HR are adjacent in the slot as they are in the pool
                self.buf[lo:lo + 51 * h * w].copy_(slot[:51 * h * w], non_blocking=True)

        with ReadAhead(len(items), read, lambda: torch.empty(slot_bytes, dtype=torch.uint8, pin_memory=True), n_readers, name="ff-pool-reader") as reads:
            for i, slot, _ in reads:                                  # arrival order: every image has its own place in the pool
                upload(i, slot)
                reads.release(slot, cache.recorded_event())
        torch.cuda.synchronize(self.dev)

    def __len__(self) -> int:
        return len(self.sizes)

    def image(self, i: int) -> Tuple[T, T]:
        """(lr_u8 [h,w,3], hr_u8 [4h,4w,3]): views of image i inside the pool."""
        (h, w), (lo, ho) = self.sizes[i], (int(v) for v in self.offsets[i])
        return self.buf[lo:lo + 3 * h * w].view(h, w, 3), self.buf[ho:ho + 48 * h * w].view(4 * h, 4 * w, 3)


class LiveEpoch:
    """Micro-batches cut from an ImagePool with the experts run on each, epoch by epoch; interchangeable with CachedEpoch in
    train_epoch and fit.

        data = LiveEpoch(model, pool, batch_size=14, repeat_factor=6, augment=True, seed=0, overlap=True)
        for lr, hr, outs, feats in data.batches(epoch): ...           # device tensors, len(data) of them
        data.close()

    An epoch uploads its descriptor table (live_plan -> int64 [nb, B, 8]) once; a micro-batch is then ONE ops.sample_pairs_u8 launch
    that writes the augmented patches straight into the expert graph's input, and one replay of that graph
    (model.experts_with_features(lr, streams=True) for [B,3,p,p], captured here, before any thread of the caller's exists, in the
    process's contraction mode ops.gemm_mode()).  The four yielded objects are static buffers of a lane: they hold a micro-batch until
    the next but `lanes - 1` is asked for, and the consumer reads them on the stream that asked (train_epoch does).
    overlap=True: two lanes, each with its own captured graph and buffers; the sampler launch and the replay of micro-batch n + 1 are
    queued on a side stream before micro-batch n is handed out, so they run beside the step the host is still launching.  Events
    order every reuse: the asking stream waits for a lane's replay, the side stream waits until the consumer of a lane's previous
    micro-batch has queued its work (known when it asks for the next one).  The tensors hold the bits of overlap=False.
    color_jitter: None (nothing changes), True (the reference's defaults, JITTER_DEFAULTS) or a dict with any of {prob, brightness,
    contrast, saturation}: the epoch's jitter table (live_jitter_plan -> fp32 [nb, B, 4]) is uploaded once as well, and
    ops.color_jitter_pairs runs in place on the lane's lr / hr between the sampler launch and the replay, on the same stream -- the
    experts and the fusion stack both see the jittered LR, as in the reference.  Independent of `augment`.
    Nothing is read from disk during an epoch, so `wait_s` stays 0.  close() destroys the graphs explicitly."""

    def __init__(self, model, pool: ImagePool, batch_size: int, repeat_factor: int = 6, augment: bool = True, seed: int = 0, overlap: bool = True,
                 shuffle: bool = True, color_jitter=None):
        self.model, self.pool, self.B, self.repeat = model, pool, int(batch_size), int(repeat_factor)
        self.augment, self.seed, self.shuffle, self.overlap = bool(augment), int(seed), shuffle, bool(overlap)
        if color_jitter is None or color_jitter is False:
            self.jitter = None
        else:
            extra = {} if color_jitter is True else dict(color_jitter)
            if set(extra) - set(JITTER_DEFAULTS):
                raise _lib.FFError(f"LiveEpoch: color_jitter takes {sorted(JITTER_DEFAULTS)}, got {sorted(extra)}")
            self.jitter = dict(JITTER_DEFAULTS, **extra)
            live_jitter_plan(0, 1, 0, 0, **self.jitter)               # the ranges are checked here, not in the first epoch
        if self.B < 1 or self.repeat < 1:
            raise _lib.FFError(f"LiveEpoch: batch_size and repeat_factor must be >= 1, got {batch_size}, {repeat_factor}")
        if len(pool) * self.repeat < self.B:
            raise _lib.FFError(f"LiveEpoch: {len(pool)} images x repeat {self.repeat} do not fill one batch of {self.B} (drop_last)")
        if torch.device(model.dev) != pool.dev:
            raise _lib.FFError(f"LiveEpoch: the model is on {model.dev}, the pool on {pool.dev}")
        self.dev = pool.dev
        self.wait_s = 0.0
        self._lanes = []
        p = pool.patch
        with torch.cuda.device(self.dev):
            try:
                for k in range(2 if self.overlap else 1):
                    ge = cache._GraphedExperts(model, p, (), tag=("live", id(self), k))
                    self._lanes.append({"experts": ge})
                    _, graph, lr, outs, feats = ge.prepare(self.B)
                    self._lanes[-1].update(graph=graph, lr=lr, outs=outs, feats=feats, ready=torch.cuda.Event(), consumed=None,
                                           hr=torch.empty((self.B, 3, 4 * p, 4 * p), device=self.dev, dtype=torch.float32))
            except BaseException:
                self.close()
                raise
            self._side = torch.cuda.Stream(device=self.dev) if self.overlap else None

    def __len__(self) -> int:
        return len(self.pool) * self.repeat // self.B

    def plan(self, epoch: int):
        return live_plan(self.pool.sizes, self.repeat, self.B, self.pool.patch, self.seed, epoch, self.augment, self.shuffle)

    def descriptors(self, epoch: int) -> np.ndarray:
        """The epoch's sampler table, int64 [nb, B, 8] = {lr_off, hr_off, h, w, top, left, code, 0} (ops.sample_pairs_u8)."""
        idx, top, left, codes = self.plan(epoch)
        img = idx % len(self.pool)
        d = np.zeros(idx.shape + (8,), dtype=np.int64)
        d[..., 0:2] = self.pool.offsets[img]
        d[..., 2:4] = np.asarray(self.pool.sizes, dtype=np.int64)[img]
        d[..., 4], d[..., 5], d[..., 6] = top, left, codes
        return d

    def jitter_table(self, epoch: int) -> Optional[np.ndarray]:
        """The epoch's colour-jitter table, fp32 [nb, B, 4] = {apply, bf, cf, sf} (ops.color_jitter_pairs); None without color_jitter."""
        return None if self.jitter is None else live_jitter_plan(len(self), self.B, self.seed, epoch, **self.jitter)

    def batches(self, epoch: int):
        from . import ops
        if not self._lanes:
            raise _lib.FFError("LiveEpoch: closed")
        desc = self.descriptors(epoch)
        jit = self.jitter_table(epoch)
        nb, p, lanes = desc.shape[0], self.pool.patch, self._lanes
        with torch.cuda.device(self.dev):
            main = torch.cuda.current_stream()
            desc_dev = torch.from_numpy(desc).to(self.dev)            # ONE upload per epoch
            jit_dev = None if jit is None else torch.from_numpy(jit).to(self.dev)
            side = self._side if self.overlap else main
            if self.overlap:
                side.wait_stream(main)                                # the tables, and whatever the caller queued before the epoch
                desc_dev.record_stream(side)
                if jit_dev is not None:
                    jit_dev.record_stream(side)

            def launch(b):                                            # sampler + expert replay of micro-batch b, on `side`
                L = lanes[b % len(lanes)]
                if self.overlap and L["consumed"] is not None:
                    side.wait_event(L["consumed"])                    # the lane's previous micro-batch has been read
                with torch.cuda.stream(side):
                    ops.sample_pairs_u8(self.pool.buf, desc[b], p, desc_dev=desc_dev[b], out=(L["lr"], L["hr"]))
                    if jit is not None:
                        ops.color_jitter_pairs(L["lr"], L["hr"], jit[b], table_dev=jit_dev[b])
                    L["graph"].replay()
                    if self.overlap:
                        L["ready"].record(side)

            try:
                if self.overlap and nb:
                    launch(0)
                for b in range(nb):
                    if not self.overlap:
                        launch(b)
                    elif b + 1 < nb:
                        launch(b + 1)                                 # queued before step b is: it runs beside that step
                    L = lanes[b % len(lanes)]
                    if self.overlap:
                        main.wait_event(L["ready"])
                    yield L["lr"], L["hr"], L["outs"], L["feats"]
                    if self.overlap:                                  # the consumer is back: its reads of this lane are queued on `main`
                        L["consumed"] = torch.cuda.Event()
                        L["consumed"].record(main)
            finally:
                if self.overlap:
                    main.wait_stream(side)                            # an abandoned epoch leaves nothing running beside the caller
                    for L in lanes:
                        L["consumed"] = None

    def close(self):
        lanes, self._lanes = self._lanes, []
        if lanes:
            torch.cuda.synchronize(self.dev)
        for L in lanes:
            L["experts"].close()


@torch.no_grad()
def live_val_samples(model, hr_dir: str, lr_dir: Optional[str] = None, patch: int = 64) -> List[dict]:
    """The validation set of a live run, computed once (the experts are frozen): per image the centre patch and the three expert
    images, dicts in cache.read_sample's shape {lr [3,p,p], hr [3,4p,4p], expert_imgs, filename} on the host.  No features: the
    eval path skips the collaborative block (enhanced_fusion.py:331, 359-362).  validate() takes the list as it is; its `skipped`
    counts the images smaller than the patch."""
    from . import ops
    with torch.cuda.device(model.dev):
        pool = ImagePool(hr_dir, lr_dir, patch=patch, device=model.dev, readers=4)
        out = ValSamples()
        out.skipped = pool.skipped
        for i, stem in enumerate(pool.stems):
            h, w = pool.sizes[i]
            lr_u8, hr_u8 = pool.image(i)
            lr, hr = ops.crop_pairs_u8(lr_u8.clone(), hr_u8.clone(), cache.crop_plan(h, w, patch, 1, 0, i, center=True), patch)
            outs, _ = model.experts_with_features(lr, streams=True)
            out.append({"lr": lr[0].cpu(), "hr": hr[0].cpu(), "expert_imgs": {k: outs[k][0].cpu() for k in EXPERTS}, "filename": stem})
    return out


def val_resized_shape(lr_h: int, lr_w: int, max_size: Optional[int] = 512, scale: int = 4) -> Optional[Tuple[int, int]]:
    """ValidationDataset's size rule (dataset.py:481-490) -> the LR size (h, w) an image pair is resized to, or None when it is kept:
    resized only when max(lr_h, lr_w) > max_size // scale; the longer side becomes max_size // scale and the other one
    int(other * new / longer) -- Python float division, then truncation; a square image takes the second (width) branch.  The HR
    partner goes to `scale` times that.  max_size None: never."""
    lr_h, lr_w = int(lr_h), int(lr_w)
    if max_size is None or max(lr_h, lr_w) <= int(max_size) // int(scale):
        return None
    if lr_h > lr_w:
        new_h = int(max_size) // int(scale)
        new_w = int(lr_w * new_h / lr_h)
    else:
        new_w = int(max_size) // int(scale)
        new_h = int(lr_h * new_w / lr_w)
    return new_h, new_w


class ValSamples(list):
    """The list live_val_samples / live_val_images return; `skipped` counts the pairs left out (smaller than the patch; HR not 4x the LR)."""
    skipped = 0


@torch.no_grad()
def live_val_images(model, hr_dir: str, lr_dir: Optional[str] = None, max_size: Optional[int] = 512, scale: int = 4) -> List[dict]:
    """The reference's validation set (create_dataloaders -> ValidationDataset(hr_dir, lr_dir, scale, max_size=512), dataset.py:473-506,
    what train.py:642 builds), computed once: WHOLE images, dicts in cache.read_sample's shape {lr [3,h,w], hr [3,4h,4w], expert_imgs,
    filename} on the host, no features -- validate() takes the list as it is.  Per pair: decoded as ImagePool decodes (without lr_dir
    the LR is made on the device as the pool makes it; a pair whose HR is not exactly 4x its LR is left out and counted in the
    result's `skipped`), u8 / 255, then -- only when the LR's longer side exceeds max_size // scale (val_resized_shape) -- LR and HR
    through ops.resize_cv_cubic (OpenCV's INTER_CUBIC restated, csrc/resample.hip) to (new_h, new_w) and four times that, clamp to
    [0, 1], and the three experts once on the whole LR.  max_size None: no resize.  The resize is parity unpinned (OpenCV absent)."""
    from . import ops
    from . import autograd as ag
    if int(scale) != 4:
        raise _lib.FFError(f"live_val_images: the experts are x4 networks, scale {scale} is refused")
    with torch.cuda.device(model.dev):
        pool = ImagePool(hr_dir, lr_dir, patch=1, device=model.dev, readers=4, skip_mismatched=True)
        out = ValSamples()
        out.skipped = pool.skipped
        for i, stem in enumerate(pool.stems):
            h, w = pool.sizes[i]
            lr_u8, hr_u8 = pool.image(i)
            lr, hr = ops.u8_to_f32_image(lr_u8.clone()), ops.u8_to_f32_image(hr_u8.clone())
            new = val_resized_shape(h, w, max_size, scale)
            if new is not None:
                lr = ops.resize_cv_cubic(lr, new[0], new[1])
                hr = ops.resize_cv_cubic(hr, 4 * new[0], 4 * new[1])
            lr, hr = ag.k_unary("clamp01", lr), ag.k_unary("clamp01", hr)
            outs, _ = model.experts_with_features(lr, streams=True)
            out.append({"lr": lr[0].cpu(), "hr": hr[0].cpu(), "expert_imgs": {k: outs[k][0].cpu() for k in EXPERTS}, "filename": stem})
    return out
