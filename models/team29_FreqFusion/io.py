"""NTIRE 2026 Image SR x4 -- Team 29 FreqFusion plugin, MI355X-native build.

Drop-in for the reference's models/team29_FreqFusion/io.py: same entry point
`main(model_dir, input_path, output_path, device=None)` (reference io.py:188-234), same checkpoint
locations and formats, same image I/O, same "whole image, else 128/32 overlap tiles on OOM" policy --
but `model(lr)` runs on hand-written HIP kernels (image-super-resolution-2_amd/) instead of ATen.
The device must be an MI355X: a CPU `device` raises (there is no fallback path).

What this build adds around the same contract:
  * one process per GPU: when WORLD_SIZE > 1 (torch.distributed.run, or isr2_amd.run_sharded) rank r takes a contiguous
    shard of the sorted image list (as the reference's eval.py:166-170 shards files over workers), the frozen weights are
    built by rank 0 and sent in ONE RCCL broadcast, every rank writes its own PNGs -- no per-image collective;
  * PNG decode and encode run on host threads beside the GPU (pinned uint8 staging, only uint8 crosses PCIe); the
    compute stays on the calling thread, results and file names are exactly those of the serial loop;
  * tiles (and repeated whole-image shapes) replay one captured HIP graph instead of re-launching ~1700 kernels;
  * FF_SELF_ENSEMBLE=1 (opt-in): every image runs through the eight symmetries of the square, the outputs are mapped back and
    averaged on the device (FreqFusionHIP.self_ensemble) -- about 8x the GPU time.
"""
from __future__ import annotations

import glob
import os
import sys
import time
import warnings
from collections import OrderedDict

import numpy as np
import torch
from PIL import Image

_THIS_DIR = os.path.dirname(os.path.abspath(__file__))
_PROJECT_ROOT = os.path.abspath(os.path.join(_THIS_DIR, "..", ".."))
if _PROJECT_ROOT not in sys.path:
    sys.path.insert(0, _PROJECT_ROOT)

from isr2_amd import ops  # noqa: E402
from isr2_amd.cache import pinned_u8, recorded_event  # noqa: E402
from isr2_amd.lib import FFError  # noqa: E402
from isr2_amd.model import FreqFusionHIP  # noqa: E402
from isr2_amd.parallel import shard_list, broadcast_state_dict  # noqa: E402
from isr2_amd.staging import ReadAhead, WriteBehind  # noqa: E402
from isr2_amd.weights import synth_state_dict, param_spec, HAT_PREFIX, DAT_PREFIX, NAF_PREFIX  # noqa: E402

# reference io.py:40-58 -- the flags the shipped checkpoint was trained with; this build implements exactly
# this configuration (the eval path it selects is SURVEY.md section 8a).
MODEL_CONFIG = {
    "scale": 4, "num_experts": 3, "fusion_dim": 64, "num_heads": 4, "refine_depth": 4, "refine_channels": 64,
    "num_bands": 3, "block_size": 8, "enable_hierarchical": True, "enable_multi_domain_freq": True,
    "enable_lka": True, "enable_edge_enhance": True, "enable_dynamic_selection": True,
    "enable_cross_band_attn": True, "enable_adaptive_bands": True, "enable_multi_resolution": True,
    "enable_collaborative": True,
}
EXPERT_FILES = {"hat": ("hat", "HAT-L_SRx4_ImageNet-pretrain.pth", HAT_PREFIX),
                "dat": ("dat", "DAT_x4.pth", DAT_PREFIX),
                "nafnet": ("nafnet", "NAFNet-SIDD-width64.pth", NAF_PREFIX)}
SYNTH_SEED = 1234


def _load_image(path: str, device=None) -> torch.Tensor:
    """PNG/JPEG -> [1,3,H,W] float32 in [0,1] (reference io.py:64-68).  With a device the uint8 pixels are uploaded and
    converted there (ff_u8hwc_to_f32nchw: same IEEE division by 255), so 1 byte per sample crosses PCIe instead of 4."""
    arr = np.array(Image.open(path).convert("RGB"), dtype=np.uint8)
    if device is not None and torch.device(device).type == "cuda":
        return ops.u8_to_f32_image(torch.from_numpy(arr).to(device))
    return torch.from_numpy(arr.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)


# zlib level of the written PNGs.  The reference saves with PIL's default (6); the pixels are what the challenge scores, and at level 6
# ONE 8160x5424 output costs ~35 s of a CPU core against ~3.5 s of GPU time for the image.  Level 1 (OpenCV's default) is ~6x faster
# for ~17 % larger files; FF_PNG_LEVEL=6 restores the reference's file sizes.  Decoded images are identical either way.
PNG_LEVEL = int(os.environ.get("FF_PNG_LEVEL", "1"))


def _save_image(tensor: torch.Tensor, path: str):
    """[1,3,H,W] -> clamp, *255, round-half-even, uint8 HWC PNG (reference io.py:71-76); converted on the device
    (ff_f32nchw_to_u8hwc) when the tensor lives there, so only the uint8 image is copied back."""
    if tensor.is_cuda:
        arr = ops.f32_to_u8_image(tensor).cpu().numpy()
    else:
        if tensor.dim() == 4:
            tensor = tensor.squeeze(0)
        arr = (tensor.clamp(0, 1).permute(1, 2, 0).numpy() * 255.0).round().astype(np.uint8)
    Image.fromarray(arr).save(path, format="PNG", compress_level=PNG_LEVEL)


def _tile_positions(n: int, tile: int, step: int):
    ps = list(range(0, max(n - tile + 1, 1), step))
    if ps[-1] + tile < n:
        ps.append(n - tile)
    return ps


_RAMPS = {}


def _ramp_table(st: int, blend: int, device) -> torch.Tensor:
    """The four edge-weight vectors a tile can have along one axis, [4, st] on the device, built ONCE per (tile, blend):
    row (has_prev + 2 * has_next) = ones, with a linear 0..1 ramp over the first `blend` samples when a tile precedes and
    a 1..0 ramp over the last `blend` when one follows (reference io.py:104-117)."""
    key = (st, blend, str(device))
    tab = _RAMPS.get(key)
    if tab is None:
        w = np.ones((4, st), dtype=np.float32)
        if blend > 0:
            ramp = np.linspace(0.0, 1.0, blend, dtype=np.float32)
            for v in range(4):
                if v & 1:
                    w[v, :blend] = ramp
                if v & 2:
                    w[v, -blend:] = 1 - ramp
        tab = _RAMPS[key] = torch.from_numpy(w).to(device)
    return tab


def _tiled_forward(model, lr_img, tile_size=64, overlap=8, scale=4, device="cuda"):
    """Overlap tiles with linear-ramp blending on interior edges (reference io.py:82-121).  Tiles of one shape replay one
    captured HIP graph when the model offers it (`model.graphed`); the blend weights live on the device."""
    _, _, h, w = lr_img.shape
    acc = torch.zeros(1, 3, h * scale, w * scale, device=device)
    wsum = torch.zeros(1, 1, h * scale, w * scale, device=device)
    step = tile_size - overlap
    st = tile_size * scale
    blend = min(overlap * scale, st // 4)
    ramps = _ramp_table(st, blend, device)
    run = getattr(model, "graphed", None) if os.environ.get("FF_TILE_GRAPH", "1") != "0" else None
    # Full-size tiles go through a two-deep pipeline (model.graphed_async: two captured graphs replayed on two lane streams), so the
    # small-grid tail of one tile overlaps the head of the next; results are accumulated in tile order on the current stream, so the
    # blend is bit-identical to the sequential loop.  FF_TILE_LANES=0 switches it off.
    run_async = getattr(model, "graphed_async", None) if run is not None and os.environ.get("FF_TILE_LANES", "1") != "0" else None
    pend = [None, None]

    def blend_in(sr_tile, y, x):
        th, tw = sr_tile.shape[-2:]
        wy = ramps[(1 if y > 0 else 0) + (2 if y + tile_size < h else 0)]
        wx = ramps[(1 if x > 0 else 0) + (2 if x + tile_size < w else 0)]
        ops.tile_accum(sr_tile, wy[:th], wx[:tw], acc, wsum, y * scale, x * scale)

    def consume(lane):
        if pend[lane] is not None:
            out, ev, y, x = pend[lane]
            torch.cuda.current_stream().wait_event(ev)
            blend_in(out, y, x)
            pend[lane] = None

    n = 0
    for y in _tile_positions(h, tile_size, step):
        for x in _tile_positions(w, tile_size, step):
            lr_tile = lr_img[:, :, y:y + tile_size, x:x + tile_size].contiguous()
            if run_async is not None and tuple(lr_tile.shape[-2:]) == (tile_size, tile_size):
                lane = n & 1
                consume(lane)                              # tile n-2: its output buffer is about to be overwritten
                out, ev = run_async(lr_tile, lane)
                pend[lane] = (out, ev, y, x)
                n += 1
                continue
            consume(n & 1)                                 # ragged edge tile: drain in tile order, then the plain path
            consume((n + 1) & 1)
            sr_tile = run(lr_tile) if run is not None else model(lr_tile)
            blend_in(sr_tile, y, x)
    consume(n & 1)
    consume((n + 1) & 1)
    ops.tile_normalize(acc, wsum)
    return acc


def _extract_state_dict(ckpt):
    """BasicSR-style containers (reference expert_loader.py:127-143)."""
    for key in ("params_ema", "params", "state_dict", "model"):
        if isinstance(ckpt, dict) and key in ckpt:
            ckpt = ckpt[key]
            break
    return OrderedDict((k.replace("module.", ""), v) for k, v in ckpt.items())


def _allow_synth() -> bool:
    return os.environ.get("FF_ALLOW_SYNTH", "0") == "1"


def _build_state_dict(model_dir: str, pretrained_dir: str, verbose: bool = True):
    """Assemble the reference-keyed state dict: seeded synthetic values first (the stand-in for the
    reference's random init when an EXPERT file is missing -- expert_loader.py:363-368 warns and keeps the random init),
    then every tensor found in the checkpoints whose name and shape match (reference io.py:164-177,
    expert_loader.py:146-157, nafnet/__init__.py:84-115).
    The FUSION checkpoint is mandatory, as in the reference (io.py:164 `torch.load` raises on a missing file): a missing or
    empty one raises unless FF_ALLOW_SYNTH=1 opts into seeded synthetic fusion weights (tests / benchmarks)."""
    sd = synth_state_dict(SYNTH_SEED)
    shapes = {n: tuple(s) for n, s, _ in param_spec()}
    for name, (sub, fname, prefix) in EXPERT_FILES.items():
        path = os.path.join(pretrained_dir, sub, fname)
        if not os.path.exists(path):
            warnings.warn(f"[team29_FreqFusion] {name} checkpoint not found: {path} -- using seeded synthetic weights")
            continue
        src = _extract_state_dict(torch.load(path, map_location="cpu", weights_only=True))
        n = 0
        for k, v in src.items():
            kk = prefix + k
            if kk in shapes and tuple(v.shape) == shapes[kk]:
                sd[kk] = v.float()
                n += 1
        if verbose:
            print(f"[team29_FreqFusion] {name}: loaded {n} tensors from {path}")
    if model_dir and os.path.exists(model_dir):
        ckpt = torch.load(model_dir, map_location="cpu", weights_only=True)
        src = ckpt.get("model_state_dict", ckpt) if isinstance(ckpt, dict) else ckpt
        n = 0
        for k, v in src.items():
            kk = k
            for pre in ("module.", "model."):
                if kk.startswith(pre):
                    kk = kk[len(pre):]
            if kk in shapes and tuple(v.shape) == shapes[kk]:
                sd[kk] = v.float()
                n += 1
        if verbose:
            print(f"[team29_FreqFusion] Loaded {n} fusion weight tensors from checkpoint")
        if n == 0 and not _allow_synth():
            raise RuntimeError(f"[team29_FreqFusion] {model_dir}: no tensor of the checkpoint matches the model "
                               "(expected a dict with 'model_state_dict'); refusing to run on synthetic fusion weights")
    elif _allow_synth():
        warnings.warn(f"[team29_FreqFusion] fusion checkpoint not found: {model_dir} -- FF_ALLOW_SYNTH=1: seeded synthetic weights")
    else:
        raise FileNotFoundError(f"[team29_FreqFusion] fusion checkpoint not found: {model_dir} "
                                "(set FF_ALLOW_SYNTH=1 to run on seeded synthetic fusion weights)")
    return sd


def _dist_env():
    """(rank, world, local_rank) of a torch.distributed.run / run_sharded launch; (0, 1, 0) otherwise."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1, 0
    rank = int(os.environ.get("RANK", "0"))
    return rank, world, int(os.environ.get("LOCAL_RANK", str(rank)))


def _ensure_process_group(rank: int, world: int, device):
    """Join the job's process group (RCCL = backend 'nccl' on ROCm; FF_DIST_BACKEND=gloo for CPU-side rehearsals)."""
    import torch.distributed as dist
    if dist.is_initialized():
        return False
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:
        # every launcher this build ships (torch.distributed.run, isr2_amd.run_sharded, bench.py) hands the ranks ONE port
        # of the job; ranks cannot agree on a free one by themselves, and a fixed default would make two jobs on a node collide
        raise RuntimeError("[team29_FreqFusion] WORLD_SIZE > 1 but MASTER_PORT is not set: start the ranks with "
                           "torch.distributed.run or `python -m isr2_amd.run_sharded` (which picks a free port per job)")
    backend = os.environ.get("FF_DIST_BACKEND", "nccl")
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(device))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    return True


def _build_and_load(model_dir: str, device, rank: int = 0, world: int = 1):
    pretrained_dir = os.environ.get("FREQFUSION_PRETRAINED", os.path.join(_PROJECT_ROOT, "pretrained"))
    if world <= 1:
        return FreqFusionHIP(_build_state_dict(model_dir, pretrained_dir), device)
    # N > 1: rank 0 reads the checkpoints, everyone receives the 690 MB of frozen weights in ONE broadcast over xGMI
    src = _build_state_dict(model_dir, pretrained_dir, verbose=True) if rank == 0 else None
    sd = broadcast_state_dict(src, param_spec(), rank, world, torch.device(device))
    return FreqFusionHIP(sd, device)


# --------------------------------------------------------------------------------------------------------------------
# Host image pipeline: decode and encode beside the GPU
class _HostPipeline:
    """PNG decode and encode beside the GPU on isr2_amd.staging: a reader thread decodes into growable pinned uint8 slots (_decode),
    writer threads encode pinned uint8 results at PNG_LEVEL (_encode); the calling thread owns every GPU call (H2D copy, kernels,
    D2H copy)."""

    def __init__(self, paths, out_dir, device, n_slots: int = 5, n_writers: int = 4):
        self.paths, self.out_dir, self.device = list(paths), out_dir, device
        self.writes = WriteBehind(self._encode, lambda: {"buf": None}, n_writers, n_slots, name="ff-png-writer")
        self.reads = ReadAhead(len(self.paths), self._decode, lambda: {"buf": None}, n_slots=n_slots, name="ff-png-reader")

    def _decode(self, i, slot):
        arr = np.asarray(Image.open(self.paths[i]).convert("RGB"), dtype=np.uint8)
        h, w, _ = arr.shape
        pinned_u8(slot, "buf", arr.size)[:arr.size].view(h, w, 3).numpy()[...] = arr
        return h, w

    def _encode(self, slot, job):
        name, h, w = job
        Image.fromarray(slot["buf"][:h * w * 3].view(h, w, 3).numpy()).save(os.path.join(self.out_dir, name), format="PNG", compress_level=PNG_LEVEL)

    def __iter__(self):
        """Yields (path, lr [1,3,H,W] fp32 on the device) in list order."""
        for i, slot, (h, w) in self.reads:
            dev_u8 = slot["buf"][:h * w * 3].view(h, w, 3).to(self.device, non_blocking=True)
            self.reads.release(slot, recorded_event())
            yield self.paths[i], ops.u8_to_f32_image(dev_u8)

    def save(self, sr: torch.Tensor, name: str):
        """Queue `sr` [1,3,H,W] (device) for PNG encoding: converted to uint8 HWC on the device, copied to a pinned slot."""
        u8 = ops.f32_to_u8_image(sr)
        h, w, _ = u8.shape
        slot = self.writes.take()
        pinned_u8(slot, "buf", u8.numel())[:u8.numel()].view(h, w, 3).copy_(u8, non_blocking=True)
        ev = recorded_event()
        u8.record_stream(torch.cuda.current_stream())
        self.writes.submit(slot, ev, (name, h, w))

    def close(self):
        try:
            self.writes.close()
        finally:
            self.reads.close()


# Graph capture costs two extra forwards and pins an activation pool; it pays where the Python launch loop (~1400 launches) is as long
# as the GPU work -- images up to about 512 x 512 LR pixels.  A 2040 x 1356 image runs 2.9 s of GPU work per forward: launched eagerly.
GRAPH_MAX_PIXELS = int(os.environ.get("FF_GRAPH_MAX_PIXELS", str(512 * 512)))


def _forward_image(model, lr_img, img_name, device, seen_shapes):
    """Whole image, else 128/32 overlap tiles when the whole image does not fit (reference io.py:219-228).  Besides the
    allocator's 'out of memory', a kernel's own size limit (FFError, e.g. the direct-DFT row length) selects the tiles."""
    shape = tuple(lr_img.shape)
    try:
        small = shape[-1] * shape[-2] <= GRAPH_MAX_PIXELS
        if small and seen_shapes is not None and hasattr(model, "graphed") and seen_shapes.get(shape, 0) >= 1:
            sr = model.graphed(lr_img)                          # a (small) shape that repeats replays its captured graph
        else:
            sr = model(lr_img)
        if seen_shapes is not None:
            seen_shapes[shape] = seen_shapes.get(shape, 0) + 1
        return sr
    except RuntimeError as e:                                    # torch.cuda.OutOfMemoryError and FFError are RuntimeErrors
        msg = str(e).lower()
        if "out of memory" in msg or (isinstance(e, FFError) and ("too large" in msg or "exceeds" in msg or "limit" in msg)):
            if torch.device(device).type == "cuda":
                torch.cuda.empty_cache()
            print(f"  OOM on {img_name}, switching to tiled inference (128px)...")
            return _tiled_forward(model, lr_img, tile_size=128, overlap=32, scale=4, device=device)
        raise


def _self_ensemble_on() -> bool:
    """FF_SELF_ENSEMBLE: absent, empty or 0 = one pass per image; 1 (or 8) = the x8 geometric self-ensemble.  Read by main()."""
    v = os.environ.get("FF_SELF_ENSEMBLE", "").strip()
    if v in ("", "0"):
        return False
    if v in ("1", "8"):
        return True
    raise ValueError(f"[team29_FreqFusion] FF_SELF_ENSEMBLE={v!r}: expected 0, 1 or 8")


def _forward_image_x8(model, lr_img, img_name, device, seen_shapes):
    """x8 geometric self-ensemble of one image (FreqFusionHIP.self_ensemble: the mean of the eight symmetries' outputs, mapped back
    and added on the device).  Every variant goes through _forward_image, so each keeps the whole-image-first policy, the graph
    replay of repeated small shapes and the fallback to 128/32 tiles.  An h x w image brings TWO shapes, h x w and w x h, four
    variants each: both are counted in seen_shapes, so from the second variant of an orientation on its graph is replayed."""
    h, w = lr_img.shape[-2:]
    if seen_shapes is not None and h != w and getattr(model, "max_graphs", 2) < 2:
        seen_shapes = None                                       # one graph slot: the two orientations would evict each other per variant
    return model.self_ensemble(lr_img, run=lambda t: _forward_image(model, t, img_name, device, seen_shapes))


@torch.no_grad()
def main(model_dir: str, input_path: str, output_path: str, device=None):
    """NTIRE2026 official interface (reference io.py:188-234)."""
    rank, world, local_rank = _dist_env()
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    device = torch.device(device)
    if world > 1 and device.type == "cuda":
        device = torch.device("cuda", local_rank % max(torch.cuda.device_count(), 1))
        torch.cuda.set_device(device)
    tag = f"[team29_FreqFusion r{rank}/{world}]" if world > 1 else "[team29_FreqFusion]"
    print(f"{tag} Device: {device}")
    own_pg = _ensure_process_group(rank, world, device) if world > 1 else False
    model = _build_and_load(model_dir, device, rank, world)
    forward_image = _forward_image
    if _self_ensemble_on():
        forward_image = _forward_image_x8
        print(f"{tag} Self-ensemble: on (8 symmetries per image, outputs mapped back and averaged; about 8x the compute)")

    input_imgs = sorted(glob.glob(os.path.join(input_path, "*.[pP][nN][gG]")))
    if not input_imgs:
        input_imgs = sorted(glob.glob(os.path.join(input_path, "*.[jJ][pP]*[gG]")))
    print(f"{tag} Found {len(input_imgs)} images in {input_path}")
    os.makedirs(output_path, exist_ok=True)
    mine = shard_list(input_imgs, rank, world)                  # contiguous shard of the sorted list; whole images per rank
    if world > 1:
        print(f"{tag} this rank processes {len(mine)} of them")

    t0 = time.perf_counter()
    if os.environ.get("FF_IO_THREADS", "1") == "0" or device.type != "cuda":   # the reference's serial loop, kept for A/B timing
        for img_path in mine:
            img_name = os.path.basename(img_path)
            lr_img = _load_image(img_path, device)
            sr_img = forward_image(model, lr_img, img_name, device, None)
            _save_image(sr_img, os.path.join(output_path, img_name))
            del sr_img, lr_img
    else:
        seen = {}
        pipe = _HostPipeline(mine, output_path, device)
        try:
            for img_path, lr_img in pipe:
                img_name = os.path.basename(img_path)
                sr_img = forward_image(model, lr_img, img_name, device, seen)
                pipe.save(sr_img, img_name)
                del sr_img, lr_img
        finally:
            pipe.close()
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        stats = torch.tensor([float(len(mine)), dt], device=device, dtype=torch.float64)
        gathered = [torch.zeros_like(stats) for _ in range(world)]
        dist.all_gather(gathered, stats)                         # end-of-run bookkeeping only (counts and wall time)
        if rank == 0:
            tot = int(sum(float(g[0]) for g in gathered))
            print(f"{tag} all ranks: {tot} images, slowest rank {max(float(g[1]) for g in gathered):.2f} s")
            assert tot == len(input_imgs), (tot, len(input_imgs))
        if own_pg:
            dist.destroy_process_group()
    print(f"{tag} Done. {len(mine)} images saved to {output_path}")
