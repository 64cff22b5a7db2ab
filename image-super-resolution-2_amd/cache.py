"""Cached-expert feature files: the on-disk contract of the reference's CachedSRDataset
(src/data/cached_dataset.py:8-25 layout, :135-200 reader) and an extractor that fills it from the HIP experts.

    {cache_dir}/{stem}_hat_part.pt    {'outputs': {'hat': [1,3,4h,4w]}, 'features': {'hat': [1,180,h,w]},
                                       'lr': [3,h,w], 'hr': [3,4h,4w], 'filename': stem}
    {cache_dir}/{stem}_rest_part.pt   {'outputs': {'dat', 'nafnet'}, 'features': {'dat': [1,180,h,w], 'nafnet': [1,64,h,w]},
                                       'filename': stem}

Plain `torch.save` dicts of CPU float32 tensors: the reference's reader loads them unchanged (its `_normalize_keys` passes
hat / dat / nafnet through, `:160-175` squeezes the batch dimension).  The frozen experts are the expensive 95 % of the path;
writing their outputs once is what lets the fusion-only training step (8f rank 1) skip them.

extract() fills a directory from ready-made (stem, lr, hr) tensors, one at a time.  build_from_folders() starts at image folders:
crop_plan() says which patches, the device cuts them (and makes the LR images of HR-only data sets), host threads decode and write
beside the GPU (`python -m isr2_amd.build_cache`).
"""
from __future__ import annotations

import os
from typing import Dict, Iterable, Optional, Tuple

import torch

T = torch.Tensor
PRIMARY_SUFFIX, REST_SUFFIX = "_hat_part.pt", "_rest_part.pt"
EXPERTS = ("hat", "dat", "nafnet")
FIELDS = ("lr", "hr") + tuple("out_" + k for k in EXPERTS) + tuple("feat_" + k for k in EXPERTS)      # the eight tensors of a cached sample


def sample_fields(sample: dict) -> Dict[str, T]:
    """The eight tensors of a read_sample dict under FIELDS' names, in FIELDS' order."""
    return dict(zip(FIELDS, (sample["lr"], sample["hr"], *(sample["expert_imgs"][k] for k in EXPERTS), *(sample["expert_feats"][k] for k in EXPERTS))))


def fields_batch(v: Dict[str, T]) -> Tuple[T, T, Dict[str, T], Dict[str, T]]:
    """The inverse: {field: tensor} of a sample or a batch -> (lr, hr, outs, feats), the arguments of write_sample and of a training step."""
    return v["lr"], v["hr"], {k: v["out_" + k] for k in EXPERTS}, {k: v["feat_" + k] for k in EXPERTS}


def fields_sample(v: Dict[str, T], filename: str) -> dict:
    """{field: tensor} of one sample -> the dict read_sample returns."""
    lr, hr, outs, feats = fields_batch(v)
    return {"lr": lr, "hr": hr, "expert_imgs": outs, "expert_feats": feats, "filename": filename}


def write_sample(cache_dir: str, stem: str, lr: T, hr: T, outputs: Dict[str, T], features: Dict[str, T]) -> Tuple[str, str]:
    """One training sample -> the two part files.  lr [3,h,w] / hr [3,4h,4w] (or with a leading batch dim of 1)."""
    os.makedirs(cache_dir, exist_ok=True)
    cpu = lambda t: t.detach().to("cpu", torch.float32).contiguous()      # noqa: E731
    sq = lambda t: t.squeeze(0) if t.dim() == 4 else t                    # noqa: E731
    for k in EXPERTS:
        if k not in outputs or k not in features:
            raise KeyError(f"cache sample {stem}: missing expert {k}")
    p1 = os.path.join(cache_dir, stem + PRIMARY_SUFFIX)
    p2 = os.path.join(cache_dir, stem + REST_SUFFIX)
    torch.save({"outputs": {"hat": cpu(outputs["hat"])}, "features": {"hat": cpu(features["hat"])},
                "lr": cpu(sq(lr)), "hr": cpu(sq(hr)), "filename": stem}, p1)
    torch.save({"outputs": {k: cpu(outputs[k]) for k in ("dat", "nafnet")},
                "features": {k: cpu(features[k]) for k in ("dat", "nafnet")}, "filename": stem}, p2)
    return p1, p2


def read_sample(cache_dir: str, stem: str, load_features: bool = True) -> dict:
    """What CachedSRDataset.__getitem__ returns without augmentation (cached_dataset.py:135-200): lr, hr, expert_imgs
    (batch dim squeezed), expert_feats, filename.  Tensors only: loaded with weights_only=True."""
    a = torch.load(os.path.join(cache_dir, stem + PRIMARY_SUFFIX), weights_only=True)
    b = torch.load(os.path.join(cache_dir, stem + REST_SUFFIX), weights_only=True)
    sq = lambda t: t.squeeze(0) if t.dim() == 4 else t                    # noqa: E731
    imgs = {k: sq(v) for d in (a["outputs"], b["outputs"]) for k, v in d.items()}
    res = {"lr": a["lr"], "hr": a["hr"], "expert_imgs": imgs, "filename": stem}
    if load_features:
        res["expert_feats"] = {k: sq(v) for d in (a.get("features", {}), b.get("features", {})) for k, v in d.items()}
    return res


def list_stems(cache_dir: str):
    return sorted(f[:-len(PRIMARY_SUFFIX)] for f in os.listdir(cache_dir) if f.endswith(PRIMARY_SUFFIX)
                  and os.path.exists(os.path.join(cache_dir, f[:-len(PRIMARY_SUFFIX)] + REST_SUFFIX)))


@torch.no_grad()
def extract(model, samples: Iterable[Tuple[str, T, Optional[T]]], cache_dir: str) -> int:
    """Run the HIP experts (model.experts_with_features = the reference's forward_all_with_hooks) over (stem, lr [1,3,h,w] or
    [3,h,w], hr or None) samples and write the cache files.  Returns the number of samples written."""
    n = 0
    for stem, lr, hr in samples:
        lr4 = lr if lr.dim() == 4 else lr.unsqueeze(0)
        outs, feats = model.experts_with_features(lr4)
        if hr is None:
            hr = torch.zeros(3, 4 * lr4.shape[-2], 4 * lr4.shape[-1])
        write_sample(cache_dir, stem, lr4, hr, outs, feats)
        n += 1
    return n


# ---- from image folders to a cache directory --------------------------------------------------------------------------------------
IMAGE_EXTS = (".png", ".jpg", ".jpeg", ".bmp")
_PLAN_TRIES = 64


def crop_plan(lr_h: int, lr_w: int, patch: int, crops: int, seed: int, image_index: int, center: bool = False):
    """LR (top, left) of the patches cut from image number `image_index` of a data set: a pure function of its arguments.
    center=True: the single centred position of the reference's non-augmented branch (dataset.py:282-296).  Otherwise `crops`
    positions, top uniform in [0, lr_h - patch] and left uniform in [0, lr_w - patch] (PairedRandomCrop, augmentations.py:77-83), from a
    random.Random seeded by (seed, image_index); a repeated position is redrawn (up to 64 tries) while the image has at least `crops`
    distinct positions.  An image smaller than the patch gives []."""
    import random
    lr_h, lr_w, p, crops = int(lr_h), int(lr_w), int(patch), int(crops)
    if p < 1 or lr_h < p or lr_w < p:
        return []
    if center:
        return [((lr_h - p) // 2, (lr_w - p) // 2)]
    rng = random.Random(((int(seed) & 0xFFFFFFFF) << 32) | (int(image_index) & 0xFFFFFFFF))
    n_pos = (lr_h - p + 1) * (lr_w - p + 1)
    plan = []
    for _ in range(crops):
        pos = (rng.randint(0, lr_h - p), rng.randint(0, lr_w - p))
        tries = 0
        while n_pos >= crops and pos in plan and tries < _PLAN_TRIES:
            pos = (rng.randint(0, lr_h - p), rng.randint(0, lr_w - p))
            tries += 1
        plan.append(pos)
    return plan


def _image_stems(folder: str) -> Dict[str, str]:
    out = {}
    for f in sorted(os.listdir(folder)):
        stem, ext = os.path.splitext(f)
        if ext.lower() in IMAGE_EXTS and stem not in out:
            out[stem] = os.path.join(folder, f)
    return out


def list_pairs(hr_dir: str, lr_dir: Optional[str] = None):
    """-> [(stem, hr_path, lr_path or None)] sorted by stem: the images of hr_dir, each with its partner of the same stem in lr_dir.
    An image without a partner, in either folder, is a FileNotFoundError naming it."""
    hr_files = _image_stems(hr_dir)
    lr_files = {} if lr_dir is None else _image_stems(lr_dir)
    missing = sorted(set(hr_files) ^ set(lr_files)) if lr_dir is not None else []
    if missing:
        raise FileNotFoundError(f"{missing[0]} has no partner in {lr_dir if missing[0] in hr_files else hr_dir}")
    return [(stem, hr_files[stem], lr_files.get(stem)) for stem in sorted(hr_files)]


def recorded_event() -> "torch.cuda.Event":
    """An event recorded on the current stream: behind the copies just queued out of (or into) a staging slot."""
    ev = torch.cuda.Event()
    ev.record()
    return ev


def pinned_u8(slot: dict, key: str, nbytes: int) -> T:
    """slot[key]: a pinned uint8 buffer of at least nbytes, grown (never below 1 MiB) when an image needs more."""
    if slot[key] is None or slot[key].numel() < nbytes:
        slot[key] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
    return slot[key]


class _BuildPipeline:
    """Host side of build_from_folders on isr2_amd.staging: one reader decodes the images into pinned uint8 slots (_read), writers run
    write_sample from pinned result slots and save the optional LR PNGs (_write); the calling thread owns every GPU call."""

    def __init__(self, items, out_dir, tmp_dir, patch, hr_only, write_lr, device, n_writers, n_in_slots=3):
        from .staging import ReadAhead, WriteBehind
        self.items, self.out_dir, self.tmp_dir, self.patch, self.hr_only = items, out_dir, tmp_dir, patch, hr_only
        self.write_lr, self.device = write_lr, device
        self.written = 0
        p = patch
        img, feat = (1, 3, 4 * p, 4 * p), (1, 180, p, p)
        shapes = dict(zip(FIELDS, ((1, 3, p, p), (3, 4 * p, 4 * p), img, img, img, feat, feat, (1, 64, p, p))))
        # every tensor owns its pinned storage: torch.save writes whole storages
        self.writes = WriteBehind(self._write, lambda: {k: torch.empty(s, dtype=torch.float32).pin_memory() for k, s in shapes.items()},
                                  n_writers, n_writers + 2, name="ff-cache-writer")
        self.reads = ReadAhead(len(items), self._read, lambda: {"lr": None, "hr": None}, n_slots=n_in_slots, name="ff-cache-reader")

    def _read(self, index, slot):
        import numpy as np
        from PIL import Image
        from .staging import SKIP
        stem, hr_path, lr_path = self.items[index]
        hr_img = Image.open(hr_path)
        W, H = hr_img.size
        if lr_path is None:
            H, W = H - H % 4, W - W % 4                               # HR-only: crop top-left to multiples of 4
            h, w = H // 4, W // 4
        else:
            lr_img = Image.open(lr_path)
            w, h = lr_img.size
            if (H, W) != (4 * h, 4 * w):
                raise ValueError(f"{hr_path}: HR is {H}x{W}, not exactly 4x its LR {lr_path} ({h}x{w})")
        if h < self.patch or w < self.patch:
            return SKIP
        hr = np.asarray(hr_img.convert("RGB"), dtype=np.uint8)[:H, :W]
        pinned_u8(slot, "hr", hr.size)[:hr.size].view(H, W, 3).numpy()[...] = hr
        if lr_path is not None:
            lr = np.asarray(lr_img.convert("RGB"), dtype=np.uint8)
            pinned_u8(slot, "lr", lr.size)[:lr.size].view(h, w, 3).numpy()[...] = lr
        return stem, h, w

    def _write(self, slot, job):
        if slot is None:                                              # an LR PNG, from the one-off buffer it came with
            from PIL import Image
            name, buf, h, w = job
            Image.fromarray(buf.view(h, w, 3).numpy()).save(os.path.join(self.write_lr, name + ".png"), format="PNG")
            return
        p1, p2 = write_sample(self.tmp_dir, job, *fields_batch(slot))
        os.replace(p2, os.path.join(self.out_dir, os.path.basename(p2)))    # the rest part first: a primary part file
        os.replace(p1, os.path.join(self.out_dir, os.path.basename(p1)))    # never exists without its partner

    def images(self):
        """Yields (index, stem, lr_u8 or None, hr_u8) with the uint8 images on the device, in list order."""
        for index, slot, (stem, h, w) in self.reads:
            hr_u8 = slot["hr"][:48 * h * w].view(4 * h, 4 * w, 3).to(self.device, non_blocking=True)
            lr_u8 = None if self.hr_only else slot["lr"][:3 * h * w].view(h, w, 3).to(self.device, non_blocking=True)
            self.reads.release(slot, recorded_event())
            yield index, stem, lr_u8, hr_u8

    def save_sample(self, stem, lr, hr, outs, feats):
        """Queue one patch's tensors (device) for write_sample: copied into a pinned slot, written once the copies' event is done."""
        slot = self.writes.take()
        for k, t in sample_fields({"lr": lr, "hr": hr, "expert_imgs": outs, "expert_feats": feats}).items():
            slot[k].copy_(t, non_blocking=True)
        self.writes.submit(slot, recorded_event(), stem)
        self.written += 1

    def save_png(self, stem, u8):
        h, w, _ = u8.shape
        buf = torch.empty(u8.numel(), dtype=torch.uint8).pin_memory()
        buf.view(h, w, 3).copy_(u8, non_blocking=True)
        self.writes.submit(None, recorded_event(), (stem, buf, h, w))

    def close(self):
        try:
            self.writes.close()
        finally:
            self.reads.close()


class _GraphedExperts:
    """model.experts_with_features for ONE patch shape, replayed from a HIP graph captured once per group size (the mechanism of
    FreqFusionHIP.graphed: a warm-up on a side stream, then the capture, with the buffers that outlive a forward keyed to this graph).
    A call takes lr [n,3,patch,patch]; every n it meets has a graph of its own (prepare(n) captures it ahead of time).  The returned
    tensors are the graph's static output buffers: consume them on the same stream before the next call.  Captured before the
    pipeline's threads exist, in thread-local capture mode: another thread pinning memory or waiting for an event must not end the
    capture."""

    def __init__(self, model, patch: int, sizes=(1,), tag="cache_build"):
        self.model, self.patch, self.tag = model, int(patch), tag      # tag: tells the graphs of two owners of one model apart
        self.ent = {}                                        # n -> (key, graph, static input, outputs, features)
        for n in sizes:
            self.prepare(n)

    def prepare(self, n: int):
        from . import ops
        n = int(n)
        if n in self.ent:
            return self.ent[n]
        model, patch = self.model, self.patch
        key = (id(model), self.tag, patch) + ((n,) if n > 1 else ())
        dev = model.dev
        graph = None
        ops.set_capture_key(key)
        try:
            with torch.cuda.device(dev):
                static_in = torch.zeros((n, 3, patch, patch), device=dev, dtype=torch.float32)
                cur = torch.cuda.current_stream()
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    model.experts_with_features(static_in, streams=True)
                cur.wait_stream(side)
                torch.cuda.synchronize(dev)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    outs, feats = model.experts_with_features(static_in, streams=True)
        finally:
            ops.set_capture_key(None)
        self.ent[n] = (key, graph, static_in, outs, feats)
        return self.ent[n]

    def __call__(self, lr: T):
        _, graph, static_in, outs, feats = self.prepare(lr.shape[0])
        static_in.copy_(lr, non_blocking=True)
        graph.replay()
        return outs, feats

    def close(self):
        """Destroy the graphs NOW: left to the garbage collector, a destructor may run inside a later capture, which HIP refuses."""
        from . import ops
        for key, graph, *_ in self.ent.values():
            graph.reset()
            ops.drop_persistent(key=key)
        self.ent = {}


@torch.no_grad()
def build_from_folders(model, hr_dir: str, out_dir: str, lr_dir: Optional[str] = None, patch: int = 64, crops: int = 5, seed: int = 0,
                       center: bool = False, writers: int = 4, write_lr: Optional[str] = None, graph: bool = True, batch: int = 1) -> dict:
    """Image folders -> the cache directory `python -m isr2_amd.train_cached` reads.  Images are matched by stem, in sorted order; image
    number i of that order is cut at crop_plan(h, w, patch, crops, seed, i, center) and patch k is written under the stem
    `{image stem}_p{k}` (the bare image stem with center=True) -- both forms are what list_stems and the reference's reader take.

    With lr_dir every HR image must be exactly 4x its LR partner (anything else is an error naming the file).  Without it the HR
    image is cropped top-left to multiples of 4 and LR = f32_to_u8_image(resize_aa(u8_to_f32_image(hr))): the antialiased bicubic
    x1/4 quantised to the uint8 a PNG would hold (write_lr=DIR saves those PNGs), so both modes cut their patches from uint8 images.

    Per image: a reader thread decodes into pinned uint8 slots, the images are uploaded, ops.crop_pairs_u8 cuts every patch pair in one
    launch, model.experts_with_features runs per patch, the results are copied into pinned slots and `writers` threads call
    write_sample into a temporary directory and rename the two part files into place.  The expert pass makes the launches extract()
    makes, so the files hold the same bits: the three experts of a patch run on three streams, as in model.experts(), and since all
    patches have one shape the pass is captured once into a HIP graph and replayed per patch (graph=False launches it instead: the
    switch exists for the bit-for-bit comparison of the two).  Images smaller than the patch are skipped and counted.
    batch=N: the K patches of an image go through the expert pass in groups of N (model.experts_with_features on [N,3,p,p]: HAT, DAT
    and NAFNet each take the group through one launch per op, on three streams); the graph is captured for [N,3,p,p] and a
    remainder group of K % N patches has a graph of its own.  Every file holds the bits batch=1 writes; batch=1 is that path, launch
    for launch.
    A reader or writer exception ends the run and is re-raised here.

    Returns {graph, batch, images, images_skipped, patches_written, seconds: {total, decode, device, write, wait_reader, wait_writer},
    patches_per_s}: decode / write are the worker threads' busy time (write summed over the writers), device is GPU time between
    the upload and the last result copy of each image (events), the waits are the calling thread's stalls for a decoded image and
    for a free result slot (staging.ReadAhead.wait_s, WriteBehind.wait_s)."""
    import contextlib
    import shutil
    import time
    from . import ops
    from .lib import FFError
    patch, crops, writers, batch = int(patch), int(crops), int(writers), int(batch)
    if patch < 1 or crops < 1 or writers < 1 or batch < 1:
        raise FFError(f"build_from_folders: patch, crops, writers and batch must be >= 1, got {patch}, {crops}, {writers}, {batch}")
    items = list_pairs(hr_dir, lr_dir)
    os.makedirs(out_dir, exist_ok=True)
    if write_lr is not None:
        os.makedirs(write_lr, exist_ok=True)
    tmp_dir = os.path.join(out_dir, f".tmp-{os.getpid()}")
    os.makedirs(tmp_dir, exist_ok=True)
    dev = model.dev
    t_start = time.perf_counter()
    spans = []
    with torch.cuda.device(dev), contextlib.ExitStack() as stack:     # left in reverse: the pipeline, the device, the graphs, the directory
        stack.callback(shutil.rmtree, tmp_dir, ignore_errors=True)
        n_patch = 1 if center else crops                      # patches per image: whole groups of `batch`, then the remainder
        sizes = sorted({min(batch, n_patch)} | ({n_patch % batch} if n_patch % batch else set()))
        experts = _GraphedExperts(model, patch, sizes) if graph else (lambda t: model.experts_with_features(t, streams=True))
        if graph:
            stack.callback(experts.close)
        stack.callback(torch.cuda.synchronize, dev)
        pipe = _BuildPipeline(items, out_dir, tmp_dir, patch, lr_dir is None, write_lr, dev, writers)
        stack.callback(pipe.close)                            # a reader's or writer's exception is re-raised here at the latest
        for index, stem, lr_u8, hr_u8 in pipe.images():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if lr_u8 is None:
                h, w = hr_u8.shape[0] // 4, hr_u8.shape[1] // 4
                lr_u8 = ops.f32_to_u8_image(ops.resize_aa(ops.u8_to_f32_image(hr_u8), (h, w)))
                if write_lr is not None:
                    pipe.save_png(stem, lr_u8)
            plan = crop_plan(lr_u8.shape[0], lr_u8.shape[1], patch, crops, seed, index, center)
            lr, hr = ops.crop_pairs_u8(lr_u8, hr_u8, plan, patch)
            for k0 in range(0, len(plan), batch):
                lr_g = lr[k0:k0 + batch]
                if lr_g.data_ptr() % 16:                          # odd patch sizes: the kernels take 16-byte aligned images
                    lr_g = lr_g.clone()
                outs, feats = experts(lr_g)
                for j in range(lr_g.shape[0]):
                    pipe.save_sample(stem if center else f"{stem}_p{k0 + j}", lr_g[j:j + 1], hr[k0 + j],
                                     {k: v[j:j + 1] for k, v in outs.items()}, {k: v[j:j + 1] for k, v in feats.items()})
            e1.record()
            spans.append((e0, e1))
    total = time.perf_counter() - t_start
    secs = {"total": total, "decode": pipe.reads.busy_s, "device": sum(a.elapsed_time(b) for a, b in spans) / 1e3,
            "write": pipe.writes.busy_s, "wait_reader": pipe.reads.wait_s, "wait_writer": pipe.writes.wait_s}
    return {"graph": bool(graph), "batch": batch, "images": len(spans), "images_skipped": len(items) - len(spans), "patches_written": pipe.written,
            "seconds": {k: round(v, 6) for k, v in secs.items()}, "patches_per_s": pipe.written / total if total > 0 else 0.0}
