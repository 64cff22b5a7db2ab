"""Torch-tensor front-end of the C ABI (include/ff_kernels.h).

PyTorch is plumbing here: it owns device memory and the stream.  Every function below only validates
shapes/strides and forwards raw pointers to libff_hip.so; there is no PyTorch compute fallback -- a
missing library or a CPU tensor raises.
Every pointer is obtained through the operand helpers (_rows, _nhwc, _dense, _image / _images, _out), and every refusal of a call precedes its
first library call.
Tensors are fp32, channel-last.  "rows view": any tensor whose last dim is contiguous and whose
leading dims collapse to a single row stride (e.g. a channel slice t[..., a:b] of an NHWC buffer).
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Tuple

import torch

from . import lib as _lib

ACT = {None: 0, "none": 0, "gelu": 1, "relu": 2, "lrelu": 3, "sigmoid": 4}
T = torch.Tensor

# ---- optional per-launch instrumentation (bench.py / profiling only; None in the product path) ----------
_PROF = None          # list collecting (kernel_class, start_event, end_event, algorithmic_flops, algorithmic_bytes)
_META = [0.0, 0.0]    # [flops, bytes] noted by the wrapper currently running


def _note(flops: float = 0.0, nbytes: float = 0.0):
    _META[0] += flops
    _META[1] += nbytes


def _numel(*ts) -> float:
    """fp32-equivalent element count (a bf16 tensor counts half: _note multiplies by 4 bytes)."""
    return float(sum(t.numel() * (t.element_size() / 4.0) for t in ts if t is not None))


def _instrument(fn):
    """Decorator of the wrappers bench.py's per-kernel-class breakdown keys on (by __name__)."""
    @functools.wraps(fn)
    def wrapped(*a, **k):
        if _PROF is None:
            return fn(*a, **k)
        _META[0] = _META[1] = 0.0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn(*a, **k)
        e1.record()
        _PROF.append((fn.__name__, e0, e1, _META[0], _META[1]))
        return r
    return wrapped


class profile:
    """with ops.profile() as p: ...  -> p.records() = [(kernel_class, ms, flops, bytes)] (events on the current stream)."""

    def __enter__(self):
        global _PROF
        self._rec = []
        _PROF = self._rec
        return self

    def __exit__(self, *exc):
        global _PROF
        _PROF = None
        torch.cuda.synchronize()

    def records(self):
        return [(n, e0.elapsed_time(e1), f, b) for n, e0, e1, f, b in self._rec]


def _L():
    return _lib.load()


# ---- contraction precision ---------------------------------------------------------------------------
# "f32"    : v_mfma_f32_32x32x2_f32, exact fp32 fma chain (parity mode, 157 TFLOP/s ceiling)
# "bf16x3" : split-operand bf16 MFMA, 3 terms, fp32-grade results (default; 833 TFLOP/s algorithmic ceiling)
# "bf16x2" : exact activations x bf16 weights;  "bf16": plain bf16 operands, fp32 accumulate
import os as _os

GEMM_MODES = {"f32": 0, "bf16": 1, "bf16x2": 2, "bf16x3": 3}
_GEMM_MODE = _os.environ.get("FF_GEMM", "bf16x3")


def set_gemm_mode(mode: str):
    global _GEMM_MODE
    if mode not in GEMM_MODES:
        raise _lib.FFError(f"unknown GEMM mode {mode!r}; expected one of {sorted(GEMM_MODES)}")
    _GEMM_MODE = mode


def _nterms() -> int:
    """MFMA terms per product of the fused token / halo / NAFNet kernels: 3 (split bf16, fp32-grade) or 1 (plain bf16)."""
    if _GEMM_MODE not in ("bf16x3", "bf16"):
        raise _lib.FFError(f"the fused bf16 kernels exist for the 'bf16x3' and 'bf16' contraction modes, not {_GEMM_MODE!r}")
    return 3 if _GEMM_MODE == "bf16x3" else 1


def fused_modes() -> bool:
    """True in the contraction modes that have the fused (token-stationary, window-resident, LDS-resident 3x3) kernels."""
    return _GEMM_MODE in ("bf16x3", "bf16")


def gemm_mode() -> str:
    return _GEMM_MODE


_HALO = True     # LDS-resident 3x3 convolution (csrc/conv3x3_halo.hip); False = generic implicit GEMM, also the fallback for shapes it does not take


def set_halo(on: bool) -> None:
    global _HALO
    _HALO = bool(on)


_ROWS_GEMM = True   # plain bf16: NAFNet's deep 1x1 GEMMs read bf16 rows through ff_gemm_rows_bf16 (csrc/gemm_rows_bf16.hip); False = fp32 rows through ff_conv2d_bf16s


def set_rows_gemm(on: bool) -> None:
    global _ROWS_GEMM
    _ROWS_GEMM = bool(on)


def rows_gemm() -> bool:
    return _ROWS_GEMM


def empty_rows_bf16(shape, device) -> T:
    """bf16 activation buffer [..., C] for an intermediate whose only consumer rounds it to bf16 anyway (plain-bf16 mode); the row
    pitch is a multiple of 64 elements (128 bytes)."""
    C = int(shape[-1])
    return torch.empty(tuple(shape[:-1]) + ((C + 63) // 64 * 64,), device=device, dtype=torch.bfloat16)[..., :C]


def empty_rows(shape, device) -> T:
    """fp32 activation buffer [..., C].  The row pitch is rounded up to a multiple of 32 floats when C is not one already
    (180 -> 192, 60 -> 64, 720 -> 736): every 32-channel segment a GEMM epilogue stores is then a whole 128-byte line
    instead of straddling two.  Kernels take the pitch as their ld argument; the padding is never touched."""
    C = int(shape[-1])
    if C >= 48 and C % 32 != 0:
        return torch.empty(tuple(shape[:-1]) + ((C + 31) // 32 * 32,), device=device, dtype=torch.float32)[..., :C]
    return torch.empty(tuple(shape), device=device, dtype=torch.float32)


def empty_like_rows(x: T) -> T:
    return empty_rows(tuple(x.shape), x.device)


# Replay lane (model.graphed_async): two captured graphs of one shape may be in flight at once, so every buffer that outlives a
# forward (NAFNet's zero-padded input, the hierarchical fusion's concat buffers) is keyed by the lane that is being captured.
_LANE = 0


def lane() -> int:
    return _LANE


def set_lane(k: int) -> None:
    global _LANE
    _LANE = int(k)


# Buffers that must outlive a forward because part of them is zeroed ONCE and never written again (the hierarchical fusion's
# 76-channel concat buffers, NAFNet's zero-padded input).  Two ownership regimes:
#   * inside model._graph_for (capture key set): the buffer belongs to THAT graph entry -- its address is baked into the captured
#     launches -- and is dropped with it when the entry is evicted (drop_persistent);
#   * eager forwards (no capture key): ONE buffer per (owner, role, device), replaced and re-zeroed when the size changes, so a
#     directory of images with many distinct shapes does not accumulate a buffer per shape.
_CAPTURE_KEY = None
_PERSIST_GRAPH: Dict[tuple, Dict[tuple, T]] = {}
_PERSIST_EAGER: Dict[tuple, T] = {}


def set_capture_key(key) -> None:
    global _CAPTURE_KEY
    _CAPTURE_KEY = key


def persistent_zeros(owner: int, role: str, shape, device) -> T:
    shape = tuple(int(v) for v in shape)
    if _CAPTURE_KEY is not None:
        slot = _PERSIST_GRAPH.setdefault(_CAPTURE_KEY, {})
        k = (owner, role, shape, str(device))
        buf = slot.get(k)
        if buf is None:
            buf = slot[k] = torch.zeros(shape, device=device, dtype=torch.float32)
        return buf
    k = (owner, role, str(device))
    buf = _PERSIST_EAGER.get(k)
    if buf is None or tuple(buf.shape) != shape:
        _PERSIST_EAGER.pop(k, None)                         # release the old size before the new one is allocated
        buf = _PERSIST_EAGER[k] = torch.zeros(shape, device=device, dtype=torch.float32)
    return buf


def drop_persistent(key=None, owner: int = None) -> None:
    """Release the buffers of one evicted graph entry (key), or everything an owner object holds (owner = id(obj))."""
    if key is not None:
        _PERSIST_GRAPH.pop(key, None)
    if owner is not None:
        for slot in _PERSIST_GRAPH.values():
            for k in [k for k in slot if k[0] == owner]:
                del slot[k]
        for k in [k for k in _PERSIST_EAGER if k[0] == owner]:
            del _PERSIST_EAGER[k]


def persistent_bytes() -> int:
    n = sum(b.numel() for b in _PERSIST_EAGER.values())
    n += sum(b.numel() for slot in _PERSIST_GRAPH.values() for b in slot.values())
    return 4 * n


class PreparedWeights:
    """Kernel-side images of weight tensors (bf16 hi/lo planes, LDS tile images, interleaved bias tables), built once per weight
    and kind.  An explicit registry instead of ad-hoc attributes on the tensors: it is thread-safe, it can be enumerated (the plan
    exporter ships these images), entries die with their weight (weak references), and `clear()` releases the device memory."""

    def __init__(self):
        import threading
        self._d: Dict[Tuple[int, str], tuple] = {}
        self._lock = threading.Lock()

    def get(self, w: T, kind: str, build):
        key = (id(w), kind)
        with self._lock:
            ent = self._d.get(key)
        if ent is not None and ent[0]() is w:
            return ent[1]
        val = build()
        import weakref
        ref = weakref.ref(w, lambda _r, key=key: self._d.pop(key, None))
        with self._lock:
            self._d[key] = (ref, val)
        return val

    def peek(self, w: T, kind: str):
        ent = self._d.get((id(w), kind))
        return ent[1] if ent is not None and ent[0]() is w else None

    def put(self, w: T, kind: str, val):
        self._d.pop((id(w), kind), None)
        return self.get(w, kind, lambda: val)

    def of(self, w: T):
        """Every prepared image of this weight: [(kind, value)]."""
        with self._lock:
            return [(k[1], e[1]) for k, e in self._d.items() if k[0] == id(w) and e[0]() is w]

    def nbytes(self) -> int:
        tot = 0

        def walk(v):
            nonlocal tot
            if isinstance(v, torch.Tensor):
                tot += v.numel() * v.element_size()
            elif isinstance(v, (tuple, list)):
                for u in v:
                    walk(u)
        with self._lock:
            for e in self._d.values():
                walk(e[1])
        return tot

    def clear(self):
        with self._lock:
            self._d.clear()


PREPARED = PreparedWeights()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# ---- the operand vocabulary ----------------------------------------------------------------------------------------------------------
# Every wrapper below takes every pointer it hands to the library from one of these helpers, before its first library call.  Each takes
# the operand, its name "op.operand" and what is expected of it, and raises FFError beginning with that name or returns what the C call
# needs.  A `shape` may hold None for an extent that is free.
_F32 = (torch.float32,)
_BF16 = (torch.bfloat16,)
_F32_BF16 = (torch.float32, torch.bfloat16)
_U8 = (torch.uint8,)
_I32 = (torch.int32,)
_I64 = (torch.int64,)


def _dev(t, name: str, dtype) -> None:
    """A tensor on the device of one of the dtypes (a tuple; None = any)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (dtype is not None and t.dtype not in dtype):
        kinds = "" if dtype is None else " or ".join(str(d).replace("torch.", "") for d in dtype) + " "
        raise _lib.FFError(f"{name}: expected a CUDA(HIP) {kinds}tensor")


def _rows(t, name: str, rows: Optional[int] = None, C: Optional[int] = None, dtype=_F32, optional: bool = False):
    """Rows operand -> (ptr, ld, rows, C): a tensor whose last dim is contiguous and whose leading dims collapse to rows of stride ld,
    of `rows` rows and `C` channels where given.  optional: None -> (None, 0)."""
    if t is None and optional:
        return None, 0
    _dev(t, name, dtype)
    shp = t.shape
    c = shp[-1]
    ld = c if len(shp) == 1 else t.stride(-2)               # (a vector is one row)
    if c and t.is_contiguous():                             # the common case, without the walk over the strides
        r = t.numel() // c
    else:
        if t.stride(-1) != 1 and c != 1:
            raise _lib.FFError(f"{name}: last dim must be contiguous")
        r, expect = 1, ld
        for d in range(len(shp) - 2, -1, -1):
            if shp[d] != 1 and t.stride(d) != expect:
                raise _lib.FFError(f"{name}: leading dims do not collapse to a constant row stride {tuple(shp)} {t.stride()}")
            expect = expect * shp[d]
            r *= shp[d]
    if (rows is not None and r != rows) or (C is not None and c != C):
        raise _lib.FFError(f"{name}: shape mismatch: expected (rows, channels) = ({rows}, {C}) (None = any), got {tuple(shp)}")
    return t.data_ptr(), ld, r, c


def rows_view(t: T, name: str = "tensor") -> Tuple[int, int, int, int]:
    """-> (ptr, ld, rows, C) for an fp32 tensor whose leading dims collapse to rows of stride ld."""
    return _rows(t, name)


def _nhwc(t, name: str, shape=None, dtype=_F32, optional: bool = False):
    """NHWC operand -> (ptr, ld, B, H, W, C): a 4-D rows view, of exactly `shape` where given.  optional: None -> (None, 0)."""
    if t is None and optional:
        return None, 0
    p, ld, _, c = _rows(t, name, dtype=dtype)
    if t.dim() != 4:
        raise _lib.FFError(f"{name}: expected [B,H,W,C]")
    if shape is not None and any(e is not None and e != s for s, e in zip(t.shape, shape)):
        raise _lib.FFError(f"{name}: shape {tuple(t.shape)} != {tuple('*' if e is None else e for e in shape)}")
    return p, ld, t.shape[0], t.shape[1], t.shape[2], c


def _dense(t, name: str, dtype=_F32, n: Optional[int] = None, shape=None, optional: bool = False):
    """Vector / table / dense-tensor operand -> ptr: on the device, of `dtype`, contiguous, with exactly n elements (any shape, e.g.
    [1,C,1,1]) or of exactly `shape`.  optional: None -> None."""
    if t is None and optional:
        return None
    _dev(t, name, dtype)
    if (not t.is_contiguous() or (n is not None and t.numel() != n)
            or (shape is not None and (t.dim() != len(shape) or any(e is not None and e != s for s, e in zip(t.shape, shape))))):
        want = f"{n} elements" if shape is None else f"shape {list('*' if e is None else e for e in shape)}"
        raise _lib.FFError(f"{name}: must be a contiguous tensor" + ("" if n is None and shape is None else " of " + want)
                           + f", got shape {list(t.shape)} with strides {list(t.stride())}")
    return t.data_ptr()


def _image(t, name: str, optional: bool = False):
    """Prepared image -> ptr: what prep.py builds (pk[...] entries, PREPARED values) or a wrapper's own workspace: on the device and
    contiguous, of any dtype."""
    return _dense(t, name, None, optional=optional)


def _images(pk: dict, name: str, *keys):
    """The pointers of several entries of one prep.py dict."""
    return tuple(_image(pk[k], f"{name}.{k}") for k in keys)


def _out(out, name: str, shape, device, bf16: bool = False, kind: str = "rows"):
    """Output -> (out, ptr, ld): a fresh buffer of `shape` when out is None (kind "rows" / "nhwc": empty_rows or empty_rows_bf16; "dense":
    contiguous) -- what this module allocated itself is not validated again -- else the caller's `out` validated: fp32 (bf16: bfloat16)
    rows of prod(shape[:-1]) rows and shape[-1] channels ("rows"), an NHWC rows view of exactly `shape` ("nhwc"), or a contiguous tensor
    of exactly `shape` ("dense", ld = shape[-1])."""
    dtype = _BF16 if bf16 else _F32
    if out is None:
        if kind == "dense":
            out = torch.empty(tuple(shape), device=device, dtype=dtype[0])
        else:
            out = empty_rows_bf16(shape, device) if bf16 else empty_rows(shape, device)
        return out, out.data_ptr(), (out.stride(-2) if out.dim() > 1 else shape[-1])
    if kind == "dense":
        return out, _dense(out, name, dtype, shape=shape), shape[-1]
    if kind == "nhwc":
        p, ld, *_ = _nhwc(out, name, shape, dtype)
    else:
        p, ld, *_ = _rows(out, name, math.prod(shape[:-1]), shape[-1], dtype)
    return out, p, ld


def _split_weight(w: T, dynamic: bool, cin: int):
    """bf16 hi/lo planes [N][Kp] of a packed fp32 weight [N][taps*cin]; cached on the tensor object unless
    `dynamic`.  Per-tap padded (TAP) K layout when cin >= 32 and cin % 4 == 0, flat otherwise."""
    nterms = GEMM_MODES[_GEMM_MODE]
    cached = None if dynamic else PREPARED.peek(w, "split")
    if cached is not None and cached[4] >= nterms:
        return cached
    wp = _dense(w, "split_weight.w", shape=(None, None))
    N, K = w.shape
    if cin >= 32 and cin % 4 == 0:
        Cp = (cin + 31) // 32 * 32
        Kp = (K // cin) * Cp
    else:
        Cp, Kp = 0, (K + 31) // 32 * 32
    hi = torch.empty((N, Kp), device=w.device, dtype=torch.bfloat16)
    lo = torch.empty((N, Kp), device=w.device, dtype=torch.bfloat16) if nterms == 3 else None
    _lib.check(_L().ff_split_bf16(wp, N, K, Kp, cin, Cp, _image(hi, "split_weight.hi"), _image(lo, "split_weight.lo", optional=True),
                                  _stream()))
    ent = (hi, lo, Kp, Cp, nterms)
    if not dynamic:
        PREPARED.put(w, "split", ent)
    return ent


class PoolPartials:
    """Per-workgroup pool partial sums written by a conv epilogue: mean[c] = inv_count * sum_r part[r][c].  vec_mlp() consumes
    them directly (ff_pool_vec_mlp: finish + channel-attention MLP in one launch); .mean() finishes them alone.
    images = B > 1 (conv2d on a batch): part holds B equal groups of rows, image b's -- those of its own single-image launch, in
    their order -- at rows b * rows_per_image ..; .mean() is [B, C]."""

    def __init__(self, part: T, C: int, inv_count: float, images: int = 1):
        if images < 1 or part.shape[0] % images:
            raise _lib.FFError(f"PoolPartials: {part.shape[0]} partial rows do not split into {images} images")
        self.part, self.C, self.inv_count, self.images = part, C, inv_count, images
        self.rows_per_image = part.shape[0] // images

    def mean(self) -> T:
        pooled = torch.empty((self.images, self.C), device=self.part.device, dtype=torch.float32)
        for b in range(self.images):                            # per image, the single-image finish (vec_mlp has the one-launch form)
            _lib.check(_L().ff_pool_finish(self.part[b * self.rows_per_image:].data_ptr(), self.rows_per_image, self.part.shape[1], self.C,
                                           self.inv_count, pooled[b:].data_ptr(), _stream()))
        return pooled


@_instrument
def conv2d(x: T, w: T, bias: Optional[T] = None, *, ksize=(1, 1), stride=(1, 1), pad=(0, 0), act=None,
           res: Optional[T] = None, mul: Optional[T] = None, alpha: float = 1.0, shuffle: int = 0,
           out: Optional[T] = None, tile_hint: int = 0, dynamic_w: bool = False, want_pool: bool = False, out_bf16: bool = False,
           per_image: bool = False):
    """x [B,H,W,Cin] (rows view), w packed [Cout, KH*KW*Cin] -> [B,Ho,Wo,Cout] (or pixel-shuffled).
    want_pool: also return the global average pool [B, Cout] of the output -> (out, pooled); the LDS-resident 3x3
    kernel produces it from its epilogue, any other path falls back to ff_pool_mean on the output.  want_pool="partials":
    the second value is a PoolPartials when the epilogue produced partial sums (else the finished pool).
    per_image (implied by want_pool; matters for B > 1 only): the batch is B independent images and every image must come out with
    the bits of its own B == 1 call -- the LDS-resident kernel goes through ff_conv3x3_halo_images (kernel form and pool partial rows
    of one image's launch), the implicit GEMM gets the tile configuration of one image's row count as its hint."""
    xp, ldi, B, H, W, Cin = _nhwc(x, "conv2d.x", dtype=_F32_BF16)
    per_image = bool(per_image or want_pool) and B > 1
    in_bf16 = x.dtype == torch.bfloat16
    KH, KW = ksize
    wp = _dense(w, "conv2d.w", shape=(None, KH * KW * Cin))
    Cout = w.shape[0]
    Ho = (H + 2 * pad[0] - KH) // stride[0] + 1
    Wo = (W + 2 * pad[1] - KW) // stride[1] + 1
    oshape = (B, Ho * 2, Wo * 2, Cout // 4) if shuffle == 2 else (B, Ho, Wo, Cout)
    if out is not None:
        out_bf16 = out.dtype == torch.bfloat16
    out, op, ldo = _out(out, "conv2d.out", oshape, x.device, bf16=out_bf16, kind="nhwc")
    halo_ok = (_HALO and _GEMM_MODE in ("bf16x3", "bf16") and (KH, KW) == (3, 3) and tuple(stride) == (1, 1) and tuple(pad) == (1, 1)
               and not dynamic_w and Cin >= 32 and Cin % 4 == 0 and ldi % 4 == 0 and xp % 16 == 0
               and (Cout <= 64 or Cin >= 128 or 128 < Cout <= 192)   # measured (profiles/r01_conv3x3_halo_vs_igemm.txt); 64 -> 256 ties
               and H * W >= 1024 and xp != op and B * H * W * ldi < 2 ** 31)
    # (the last term is the one condition that counts the whole launch: the kernel's 32-bit offsets.  A caller that batches independent
    # images keeps its batches below it -- HatHIP.forward sizes its chunks so -- and every other term is one image's.)
    if (in_bf16 or out_bf16) and not (halo_ok and _GEMM_MODE == "bf16" and shuffle == 0 and res is None):
        raise _lib.FFError("conv2d: bf16 input / output rows exist for the LDS-resident 3x3 kernel in plain-bf16 mode only")
    rp, ldr, *_ = _nhwc(res, "conv2d.res", oshape, optional=True)
    bp = _dense(bias, "conv2d.bias", n=Cout, optional=True)
    mp = _dense(mul, "conv2d.mul", n=Cout, optional=True)
    if (_GEMM_MODE != "f32" and (KH, KW) == (3, 3) and tuple(stride) == (1, 1) and tuple(pad) == (1, 1) and Cout <= 16
            and Cin * (1 if Cout == 1 else (4 if Cout <= 4 else 16)) <= 128 and shuffle == 0 and mul is None and not dynamic_w and H * W >= 4096 and xp != op):
        # small-channel tail convolutions: exact fp32 on the VALU from an LDS halo tile (csrc/conv3x3_small.hip).  Measured on
        # MI355X at 1024 x 1024: 16->3 205 -> <70 us, 8->1 160 -> <70, 16->1 204 -> <70, 32->3 166 -> 95, 6->16 173 -> 126; but
        # 64->3 202 -> 370 and 32->16 187 -> 199 (VALU-bound: Cin * CT FMAs per pixel and tap), hence the Cin * CT <= 128 rule
        from . import prep as _prep
        ws = PREPARED.get(w, "small", lambda: _prep.pack_conv3x3_small(w, Cin))
        _lib.check(_L().ff_conv3x3_small(xp, ldi, _image(ws, "conv2d.w[small]"), ws.shape[2], bp, rp, ldr, op, ldo, B, H, W, Cin, Cout, ACT[act],
                                         float(alpha), _stream()))
    elif _GEMM_MODE == "f32":
        _lib.check(_L().ff_conv2d(xp, wp, bp, mp, rp, op, B, H, W, Cin, ldi, Ho, Wo, Cout, ldo, ldr, KH, KW, stride[0], stride[1],
                                  pad[0], pad[1], ACT[act], float(alpha), shuffle, tile_hint, _stream()))
    elif halo_ok:
        from . import prep as _prep

        nt_ = _nterms()

        def _mk_halo():
            bn = _prep.halo_bn(Cout)
            return (_prep.pack_conv3x3_halo(w, Cin, bn, nt_), bn)
        img = PREPARED.get(w, "halo" if nt_ == 3 else "halo1", _mk_halo)
        imgp = _image(img[0], "conv2d.w[halo]")
        part = None
        halo_fn, rows_fn = ((_L().ff_conv3x3_halo_images, _L().ff_conv3x3_halo_images_pool_rows) if per_image else
                            (_L().ff_conv3x3_halo, _L().ff_conv3x3_halo_pool_rows))
        if want_pool and (B == 1 or per_image) and shuffle == 0 and Cout <= img[1]:
            prow = int(rows_fn(B, H, W, Cout, img[1], nt_))
            part = torch.empty((prow, img[1]), device=x.device, dtype=torch.float32)
        _lib.check(halo_fn(xp, ldi, imgp, img[1], bp, mp, rp, ldr, op, ldo, B, H, W, Cin, Cout, ACT[act], float(alpha), shuffle,
                           _dense(part, "conv2d.part", optional=True), nt_, (1 if in_bf16 else 0) | (2 if out_bf16 else 0), _stream()))
        if part is not None:
            pp = PoolPartials(part, Cout, 1.0 / float(H * W), images=B)
            _note(2.0 * B * Ho * Wo * Cout * KH * KW * Cin, 4.0 * (_numel(x, w, out, res)))
            return out, (pp if want_pool == "partials" else pp.mean())
    else:
        aligned = (ldi % 4 == 0) and (xp % 16 == 0)
        ent = _split_weight(w, dynamic_w, Cin if aligned else 0)
        hip, lop = _image(ent[0], "conv2d.w[hi]"), _image(ent[1], "conv2d.w[lo]", optional=True)
        if per_image and tile_hint <= 0:                    # the tile configuration one image's launch picks for itself
            tile_hint = int(_L().ff_conv2d_bf16s_tile(Ho * Wo, Cout, KH * KW * Cin, 1 if aligned and Cin % 4 == 0 else 0))
        _lib.check(_L().ff_conv2d_bf16s(xp, hip, lop, ent[2], ent[3], bp, mp, rp, op, B, H, W, Cin, ldi, Ho, Wo, Cout, ldo, ldr, KH, KW,
                                        stride[0], stride[1], pad[0], pad[1], ACT[act], float(alpha), shuffle, GEMM_MODES[_GEMM_MODE],
                                        tile_hint, None, _stream()))
    _note(2.0 * B * Ho * Wo * Cout * KH * KW * Cin, 4.0 * (_numel(x, w, out, res)))
    if want_pool:
        return out, pool_mean(out)
    return out


@_instrument
def linear(x: T, w: T, bias: Optional[T] = None, *, act=None, res: Optional[T] = None, mul: Optional[T] = None,
           alpha: float = 1.0, out: Optional[T] = None, dynamic_w: bool = False, kmul: Optional[T] = None,
           gate_pairs: bool = False, out_bf16: bool = False, tile_hint: int = 0, rows_gemm: bool = False,
           rows_per_image: int = 0) -> T:
    """x [..., K] rows view, w [N, K] -> [..., N].
    rows_per_image (fp32-rows route of the split-bf16 modes; 0 = the rows are one image): the rows are equal groups of this many rows, one
    independent image each, and the implicit GEMM takes the tile configuration ONE group's row count picks for itself
    (ff_conv2d_bf16s_tile), so every image has the bits of its own call.  A value that equals the row count changes nothing.  kmul [K]: scale of the input channels (W (kmul * x); split-bf16 modes).
    kmul [B, K] with B > 1: the rows are B equal groups (rows % B == 0), group b scaled by kmul[b], in one launch -- every group with
    the bits of its own call with kmul[b] (the tile configuration is taken from one group's row count).
    gate_pairs: SimpleGate in the epilogue, [..., N / 2] out with out[j] = y[2j] * y[2j+1] (rows of w interleaved by the caller).
    bf16 x (plain-bf16 mode, rows_gemm_ok shapes): ff_gemm_rows_bf16, bit-equal to the fp32-rows kernel on x.float(); out_bf16 stores
    the gated output as bf16 rows for the next such GEMM.  rows_gemm: fp32 x through the same kernel (A staged through registers; the
    only form that takes kmul), again bit-equal; without it fp32 x stays on ff_conv2d_bf16s.
    w [B, N, K] with B > 1 (dynamic_w=True, split-bf16 modes): the rows are B equal groups of a multiple of 256 rows, group b multiplied by
    w[b], in one launch (ff_conv2d_bf16s_wimages) -- every group with the bits of its own call with w[b]."""
    if w.dim() == 3 and w.shape[0] > 1:
        return _linear_wimages(x, w, bias, act=act, res=res, mul=mul, alpha=alpha, out=out, dynamic_w=dynamic_w, kmul=kmul,
                               gate_pairs=gate_pairs, out_bf16=out_bf16, tile_hint=tile_hint, rows_gemm=rows_gemm)
    if w.dim() == 3:                                         # one image: the single-weight entry
        w = w[0]
    rows_per_image = int(rows_per_image)
    if rows_per_image and (rows_per_image < 0 or x.dtype == torch.bfloat16 or rows_gemm or w.dim() == 3 or (kmul is not None and kmul.numel() != w.shape[-1])):
        raise _lib.FFError("linear: rows_per_image belongs to the fp32-rows route with one weight matrix and one kmul vector")
    if x.dtype == torch.bfloat16 or rows_gemm:
        return _linear_rows_bf16(x, w, bias, act=act, res=res, mul=mul, alpha=alpha, out=out, dynamic_w=dynamic_w, kmul=kmul,
                                 gate_pairs=gate_pairs, out_bf16=out_bf16, tile_hint=tile_hint)
    if out_bf16 or tile_hint:
        raise _lib.FFError("linear: out_bf16 / tile_hint belong to the bf16-rows route (bf16 x, or rows_gemm)")
    xp, ldi, rows, K = _rows(x, "linear.x")
    wp = _dense(w, "linear.w", shape=(None, K))
    N = w.shape[0]
    if (kmul is not None or gate_pairs) and _GEMM_MODE == "f32":
        raise _lib.FFError("linear: kmul / gate_pairs exist in the split-bf16 kernels only")
    No = N // 2 if gate_pairs else N
    out, op, ldo = _out(out, "linear.out", tuple(x.shape[:-1]) + (No,), x.device)
    rp, ldr, *_ = _rows(res, "linear.res", rows, N, optional=True)
    if rows_per_image and rows % rows_per_image:
        raise _lib.FFError(f"linear: {rows} rows are not whole images of rows_per_image = {rows_per_image} rows")
    bp = _dense(bias, "linear.bias", n=N, optional=True)
    mp = _dense(mul, "linear.mul", n=N, optional=True)
    images, kp = _kmul_images(kmul, K, rows)                 # (refusals first: nothing is launched, no weight is split, before them)
    if _GEMM_MODE == "f32":
        _lib.check(_L().ff_conv2d(xp, wp, bp, mp, rp, op, 1, 1, rows, K, ldi, 1, rows, N, ldo, ldr, 1, 1, 1, 1, 0, 0, ACT[act],
                                  float(alpha), 0, 0, _stream()))
    else:
        aligned = (ldi % 4 == 0) and (xp % 16 == 0)
        if images > 1 and (act is not None or alpha != 1.0 or gate_pairs or not aligned or K % 4 or N % 4):
            raise _lib.FFError("linear: kmul [B, K] comes with the (bias, * mul, + res) epilogue on 16-byte aligned rows only")
        ent = _split_weight(w, dynamic_w, K if aligned else 0)
        hip, lop = _image(ent[0], "linear.w[hi]"), _image(ent[1], "linear.w[lo]", optional=True)
        if images > 1:
            _lib.check(_L().ff_conv2d_bf16s_kmul_images(xp, ldi, hip, lop, ent[2], ent[3], kp, images, rows // images, bp, mp, rp, ldr,
                                                        op, ldo, rows, K, N, GEMM_MODES[_GEMM_MODE], 0, _stream()))
        else:
            hint = 0                                         # several images: the tile configuration one image's launch picks for itself
            if rows_per_image and rows_per_image != rows:
                hint = int(_L().ff_conv2d_bf16s_tile(rows_per_image, N, K, 1 if aligned and K % 4 == 0 else 0))
            _lib.check(_L().ff_conv2d_bf16s(xp, hip, lop, ent[2], ent[3], bp, mp, rp, op, 1, 1, rows, K, ldi, 1, rows, N, ldo, ldr, 1, 1,
                                            1, 1, 0, 0, ACT[act], float(alpha), 1 if gate_pairs else 0, GEMM_MODES[_GEMM_MODE], hint, kp, _stream()))
    _note(2.0 * rows * N * K, 4.0 * (rows * K + N * K + rows * No * (2 if res is not None else 1)))
    return out


def _linear_wimages(x: T, w: T, bias, *, act, res, mul, alpha, out, dynamic_w, kmul, gate_pairs, out_bf16, tile_hint, rows_gemm) -> T:
    """linear with one weight matrix per image, w [B, N, K].  Every refusal comes before the weight split and the launch."""
    _dev(w, "linear.w", _F32)
    B, N, K = w.shape
    if _GEMM_MODE == "f32" or not dynamic_w or not w.is_contiguous():
        raise _lib.FFError("linear: per-image weights [B, N, K] are contiguous dynamic weights (dynamic_w=True) of the split-bf16 modes")
    if (x.dtype != torch.float32 or rows_gemm or kmul is not None or gate_pairs or out_bf16 or tile_hint or act is not None
            or alpha != 1.0):
        raise _lib.FFError("linear: per-image weights come with fp32 rows and the (bias, * mul, + res) epilogue only")
    xp, ldi, rows, xk = _rows(x, "linear.x")
    if xk != K or rows % B or (rows // B) % 256:
        raise _lib.FFError(f"linear: per-image weights {tuple(w.shape)} need [rows, {K}] input with B = {B} equal groups of a multiple of "
                           f"256 rows, got {rows} rows of {xk}")
    if ldi % 4 or xp % 16 or K % 4 or N % 4:
        raise _lib.FFError("linear: per-image weights need 16-byte aligned rows, K % 4 == 0 and N % 4 == 0")
    out, op, ldo = _out(out, "linear.out", tuple(x.shape[:-1]) + (N,), x.device)
    if ldo % 4 or op % 16:
        raise _lib.FFError("linear: out shape mismatch (per-image weights: 16-byte aligned rows)")
    rp, ldr, *_ = _rows(res, "linear.res", rows, N, optional=True)
    if res is not None and (ldr % 4 or rp % 16):
        raise _lib.FFError("linear: res shape mismatch (per-image weights: 16-byte aligned rows)")
    bp = _dense(bias, "linear.bias", n=N, optional=True)
    mp = _dense(mul, "linear.mul", n=N, optional=True)
    ent = _split_weight(w.reshape(B * N, K), True, K)        # rows are split independently: image b's planes at [b * N, (b + 1) * N)
    hip, lop = _image(ent[0], "linear.w[hi]"), _image(ent[1], "linear.w[lo]", optional=True)
    _lib.check(_L().ff_conv2d_bf16s_wimages(xp, ldi, hip, lop, ent[2], ent[3], B, rows // B, bp, mp, rp, ldr, op, ldo, rows, K, N,
                                            GEMM_MODES[_GEMM_MODE], 0, _stream()))
    _note(2.0 * rows * N * K, 4.0 * (rows * K + B * N * K + rows * N * (2 if res is not None else 1)))
    return out


def _kmul_images(kmul: Optional[T], K: int, rows: int):
    """linear's kmul -> (images, ptr): [K] (or [1, K]) -> 1; a contiguous [B, K] matrix with B > 1 dividing the row count -> B; None ->
    (1, None); anything else raises."""
    if kmul is None:
        return 1, None
    _dev(kmul, "linear.kmul", _F32)
    if not kmul.is_contiguous() or kmul.numel() % K or (kmul.numel() != K and (kmul.dim() != 2 or kmul.shape[1] != K)):
        raise _lib.FFError(f"linear: kmul must be a contiguous [{K}] vector or [B, {K}] matrix, got {tuple(kmul.shape)}")
    images = kmul.numel() // K
    if images < 1 or rows % images:
        raise _lib.FFError(f"linear: kmul {tuple(kmul.shape)} needs a row count that B = {images} divides, got {rows} rows")
    return images, _dense(kmul, "linear.kmul", n=images * K)


def rows_gemm_ok(K: int) -> bool:
    """Shapes ff_gemm_rows_bf16 takes: whole 64-wide K chunks, so that the weight plane of _split_weight is unpadded."""
    return K % 64 == 0


def _linear_rows_bf16(x: T, w: T, bias, *, act, res, mul, alpha, out, dynamic_w, kmul, gate_pairs, out_bf16, tile_hint) -> T:
    xp, lda, rows, K = _rows(x, "linear.x", dtype=_F32_BF16)
    a32 = x.dtype == torch.float32
    _dense(w, "linear.w", shape=(None, K))
    N = w.shape[0]
    if _GEMM_MODE != "bf16" or not rows_gemm_ok(K):
        raise _lib.FFError("linear: the bf16-rows GEMM exists in plain-bf16 mode for K % 64 == 0 only")
    if kmul is not None and not a32:
        raise _lib.FFError("linear: kmul scales fp32 input rows only")
    images, kp = _kmul_images(kmul, K, rows)
    if act is not None or alpha != 1.0 or (a32 and gate_pairs) or (gate_pairs and (res is not None or mul is not None)) or out_bf16 != gate_pairs:
        raise _lib.FFError("linear: the bf16-rows GEMM has three epilogues: bias (* mul + res) -> fp32 rows, or the SimpleGate pair "
                           "product -> bf16 rows")
    No = N // 2 if gate_pairs else N
    if out is not None and (out.dtype == torch.bfloat16) != out_bf16:
        raise _lib.FFError("linear: out dtype does not match out_bf16")
    out, op, ldo = _out(out, "linear.out", tuple(x.shape[:-1]) + (No,), x.device, bf16=out_bf16)
    rp, ldr, *_ = _rows(res, "linear.res", rows, N, optional=True)
    bp = _dense(bias, "linear.bias", n=N, optional=True)
    mp = _dense(mul, "linear.mul", n=N, optional=True)
    ent = _split_weight(w, dynamic_w, K)
    hip = _image(ent[0], "linear.w[hi]")
    if images > 1:
        _lib.check(_L().ff_gemm_rows_bf16_kmul_images(xp, lda, hip, ent[2], kp, images, rows // images, bp, mp,
                                                      rp, ldr, op, ldo, rows, N, K, int(tile_hint), _stream()))
    else:
        _lib.check(_L().ff_gemm_rows_bf16(xp, 1 if a32 else 0, lda, hip, ent[2], kp, bp, mp, rp, ldr, op, ldo, rows,
                                          N, K, 1 if gate_pairs else 0, int(tile_hint), _stream()))
    _note(2.0 * rows * N * K, (4.0 if a32 else 2.0) * rows * K + 2.0 * N * K + (2.0 if out_bf16 else 4.0) * rows * No + (4.0 * rows * No if res is not None else 0.0))
    return out


@_instrument
def window_attn(qkv: T, out: T, biasT: T, *, q_off: int, k_off: int, v_off: int, o_off: int, H: int, W: int, Hp: int,
                Wp: int, win: Tuple[int, int], kwin: Tuple[int, int], shift: Tuple[int, int], use_mask: bool, heads: int,
                d: int, scale: float, rel_table: Optional[T] = None) -> T:
    qp, ldq, B, h_, w_, _ = _nhwc(qkv, "window_attn.qkv")
    if (h_, w_) != (H, W):
        raise _lib.FFError("window_attn: qkv/out spatial dims mismatch")
    op, ldo, *_ = _nhwc(out, "window_attn.out", (B, H, W, None))
    nk = kwin[0] * kwin[1]
    bp = _dense(biasT, "window_attn.biasT", shape=(heads, nk, 256))
    if q_off + heads * d > qkv.shape[-1] or k_off + heads * d > qkv.shape[-1] or v_off + heads * d > qkv.shape[-1] \
            or o_off + heads * d > out.shape[-1]:
        raise _lib.FFError("window_attn: channel offsets out of range")
    if _GEMM_MODE == "f32":
        _lib.check(_L().ff_window_attn(qp, ldq, q_off, k_off, v_off, op, ldo, o_off, bp, B, H, W, Hp, Wp, win[0],
                                       win[1], kwin[0], kwin[1], shift[0], shift[1], int(use_mask), heads, d, float(scale),
                                       _stream()))
    else:
        relp = None
        if rel_table is not None and tuple(kwin) != tuple(win):
            # overlapping keys: the rotated table of prep.pack_rel_overlap, gathered in the kernel through a per-key offset table
            n = (win[0] + kwin[0] - 1) * (win[1] + kwin[1] - 1)
            if kwin[1] % 8 or tuple(shift) != (0, 0):
                raise _lib.FFError(f"window_attn: overlapping-window rel_table must be [heads, {n}] (prep.pack_rel_overlap), kw % 8 == 0, no shift")
            relp = _dense(rel_table, "window_attn.rel_table", shape=(heads, n))
        elif rel_table is not None and tuple(kwin) == tuple(win) and win[1] & (win[1] - 1) == 0 and win[1] >= 8:
            relp = _dense(rel_table, "window_attn.rel_table", shape=(heads, (2 * win[0] - 1) * (2 * win[1] - 1)))
        from . import prep as _prep
        bq = PREPARED.get(biasT, "quad", lambda: _prep.quad_bias(biasT))          # load-time relayout, once per table
        _lib.check(_L().ff_window_attn_bf16s(qp, ldq, q_off, k_off, v_off, op, ldo, o_off, _image(bq, "window_attn.biasT[quad]"), B, H, W, Hp, Wp,
                                             win[0], win[1], kwin[0], kwin[1], shift[0], shift[1], int(use_mask), heads, d,
                                             float(scale), 1 if _GEMM_MODE == "bf16" else 3, relp, _stream()))
    nwin = B * (Hp // win[0]) * (Wp // win[1])
    _note(4.0 * nwin * heads * 256 * nk * d, 4.0 * (4.0 * B * H * W * heads * d + heads * nk * 256))
    return out


@_instrument
def ocab_attn(qkv: T, out: T, rel_rotated: T, *, q_off: int, k_off: int, v_off: int, o_off: int = 0, H: int, W: int, heads: int, d: int,
              ws: int, ows: int, scale: float) -> T:
    """HAT OCAB attention stage in one persistent-workgroup launch (plain bf16; csrc/ocab_attn.hip): 16x16 query windows against
    24x24 zero-padded key windows, bias from the rotated compact table of prep.pack_rel_overlap [heads, 39*39]."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("ocab_attn exists for the plain-bf16 contraction mode only")
    qp, ldq, B, *_ = _nhwc(qkv, "ocab_attn.qkv", (None, H, W, None))
    op, ldo, *_ = _nhwc(out, "ocab_attn.out", (B, H, W, None), _F32_BF16)
    out_bf16 = out.dtype == torch.bfloat16
    relp = _dense(rel_rotated, "ocab_attn.rel_rotated", shape=(heads, (ws + ows - 1) ** 2))
    _lib.check(_L().ff_ocab_attn(qp, ldq, q_off, k_off, v_off, op, ldo, o_off, relp, B, H, W, heads, d, ws, ows,
                                 float(scale), int(out_bf16), _stream()))
    nwin = B * (H // ws) * (W // ws)
    _note(4.0 * nwin * heads * ws * ws * ows * ows * d, 4.0 * B * H * W * heads * d * 4)
    return out


@_instrument
def ocab_attn_rows16(qkv16: T, out: T, rel_rotated: T, *, q_off: int, k_off: int, v_off: int, o_off: int = 0, H: int, W: int, heads: int,
                     d: int, ws: int, ows: int) -> T:
    """ocab_attn on the head-padded bf16 rows of token_linear_rows16 (csrc/ocab_attn.hip, ROWS16): head h of q / k / v at
    q_off / k_off / v_off + 32 h, q already scaled."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("ocab_attn_rows16 exists for the plain-bf16 contraction mode only")
    qp, ldq, B, *_ = _nhwc(qkv16, "ocab_attn_rows16.qkv", (None, H, W, None), _BF16)
    op, ldo, *_ = _nhwc(out, "ocab_attn_rows16.out", (B, H, W, None), _F32_BF16)
    out_bf16 = out.dtype == torch.bfloat16
    relp = _dense(rel_rotated, "ocab_attn_rows16.rel_rotated", shape=(heads, (ws + ows - 1) ** 2))
    if max(q_off, k_off, v_off) + heads * 32 > qkv16.shape[-1]:
        raise _lib.FFError("ocab_attn_rows16: channel offsets out of range")
    _lib.check(_L().ff_ocab_attn_rows16(qp, ldq, q_off, k_off, v_off, op, ldo, o_off, relp, B, H, W, heads, d, ws, ows,
                                        int(out_bf16), _stream()))
    nwin = B * (H // ws) * (W // ws)
    _note(4.0 * nwin * heads * ws * ws * ows * ows * d, B * H * W * heads * (2.0 * 3 * 32 + (2.0 if out_bf16 else 4.0) * d))
    return out


@_instrument
def win_attn_fused(x: T, out: T, pk: dict, rel_padded: T, *, gamma: Optional[T], beta: Optional[T], eps: float = 1e-5,
                   H: int, W: int, Hp: int, Wp: int, win: Tuple[int, int], shift: Tuple[int, int], use_mask: bool,
                   head0: int = 0, nheads: Optional[int] = None, o_off: int = 0, zero_pad: bool = False,
                   want_xn: bool = False, v_out: Optional[T] = None, v_off: int = 0):
    """LayerNorm + qkv projection + window attention of `nheads` heads in one launch (csrc/win_attn_fused.hip); pk from
    prep.pack_win_attn, rel_padded from prep.pack_win_rel.  x [B,H,W,K] rows view; out [B,H,W,>= o_off + heads*d].
    want_xn: also return the normalised rows; v_out: receives v of the processed heads at channel v_off + g*d."""
    xp, ldx, B, _, _, K = _nhwc(x, "win_attn_fused.x", (None, H, W, pk["K"]))
    op, ldo, *_ = _nhwc(out, "win_attn_fused.out", (B, H, W, None), _F32_BF16)
    out_bf16 = out.dtype == torch.bfloat16
    xn_bf16 = want_xn == "bf16"
    if (out_bf16 or xn_bf16) and _GEMM_MODE != "bf16":
        raise _lib.FFError("win_attn_fused: bf16 outputs exist for the plain-bf16 contraction mode only")
    nheads = pk["heads"] - head0 if nheads is None else nheads
    relp = _dense(rel_padded, "win_attn_fused.rel_padded", shape=(pk["heads"], 2 * win[0] - 1, None))
    if _GEMM_MODE not in ("bf16x3", "bf16"):
        raise _lib.FFError("win_attn_fused exists for the bf16 contraction modes only")
    gp = _dense(gamma, "win_attn_fused.gamma", n=K, optional=True)
    bp = _dense(beta, "win_attn_fused.beta", n=K, optional=True)
    wp, wbp = _image(pk["w"], "win_attn_fused.pk.w"), _image(pk["b"], "win_attn_fused.pk.b")
    vp, ldv, *_ = _nhwc(v_out, "win_attn_fused.v_out", (B, H, W, None), optional=True)
    xn, xnp, ldxn = None, None, 0
    if want_xn:
        xn, xnp, ldxn = _out(None, "win_attn_fused.xn", tuple(x.shape), x.device, bf16=xn_bf16)
    _lib.check(_L().ff_win_attn_fused(xp, ldx, op, ldo, o_off, gp, bp, float(eps), wp, wbp, relp, rel_padded.shape[1], rel_padded.shape[2],
                                      B, H, W, Hp, Wp, win[0], win[1], shift[0], shift[1], int(use_mask), head0, nheads, pk["d"], K,
                                      int(zero_pad), xnp, ldxn, vp, ldv, v_off, 1 if _GEMM_MODE == "bf16" else 3, int(out_bf16), int(xn_bf16),
                                      _stream()))
    nwin = B * (Hp // win[0]) * (Wp // win[1])
    _note(2.0 * nwin * 256 * K * 3 * nheads * pk["d"] + 4.0 * nwin * nheads * 256 * 256 * pk["d"],
          4.0 * B * H * W * (K * (1 + (0 if not want_xn else (0.5 if xn_bf16 else 1.0))) + nheads * pk["d"] * ((0.5 if out_bf16 else 1.0) + (1 if v_out is not None else 0))))
    return (out, xn) if want_xn else out


@_instrument
def token_mlp(x: T, gamma: T, beta: T, pk: dict, eps: float = 1e-5) -> T:
    """x + fc2(GELU(fc1(LayerNorm(x)))) in one launch (bf16x3 only); pk from prep.pack_token_mlp."""
    xp, ldx, rows, K = _rows(x, "token_mlp.x", C=pk["K"])
    if pk["N"] != K:
        raise _lib.FFError("token_mlp: shape mismatch")
    gp, bp = _dense(gamma, "token_mlp.gamma", n=K), _dense(beta, "token_mlp.beta", n=K)
    wp, b1p, b2p = _images(pk, "token_mlp.pk", "w", "b1", "b2")
    nt = _nterms()
    out, op_, ldo_ = _out(None, "token_mlp.out", tuple(x.shape), x.device)
    _lib.check(_L().ff_token_mlp(xp, ldx, op_, ldo_, rows, K, pk["ht"], pk["N"], gp, bp, float(eps), wp, b1p, b2p, nt, _stream()))
    _note(4.0 * rows * K * pk["ht"] * 32, 8.0 * rows * K)
    return out


@_instrument
def token_projmlp(att: T, x: T, pk: dict, gamma: T, beta: T, *, c2: Optional[T] = None, c2_scale: Optional[T] = None,
                  eps: float = 1e-5) -> T:
    """x1 = x + proj(att) + c2 * c2_scale; return x1 + fc2(GELU(fc1(LayerNorm(x1)))) in one launch (bf16x3); pk from
    prep.pack_token_projmlp.  c2_scale [K] (or [1,K]): one gate for every row.  c2_scale [B,K] with B = x.shape[0] > 1: one gate per image
    (ff_token_projmlp_images; every image must be a multiple of 256 rows), bit-equal to B calls on the row slices."""
    att_bf16 = isinstance(att, torch.Tensor) and att.dtype == torch.bfloat16
    c2_bf16 = c2 is not None and c2.dtype == torch.bfloat16
    if (att_bf16 or c2_bf16) and _GEMM_MODE != "bf16":
        raise _lib.FFError("token_projmlp: bf16 att / c2 rows exist for the plain-bf16 contraction mode only")
    ap, lda, rows, K = _rows(att, "token_projmlp.att", C=pk["mlp"]["K"], dtype=_F32_BF16)
    xp, ldx, *_ = _rows(x, "token_projmlp.x", rows, K)
    cp, ldc, *_ = _rows(c2, "token_projmlp.c2", rows, K, _F32_BF16, optional=True)
    if c2 is not None and c2_scale is None:
        raise _lib.FFError("token_projmlp: c2 shape mismatch")
    nimg = 1
    if c2 is not None and c2_scale.numel() != K:
        nimg = int(x.shape[0])
        if c2_scale.dim() != 2 or tuple(c2_scale.shape) != (nimg, K) or not c2_scale.is_contiguous() or rows % nimg:
            raise _lib.FFError(f"token_projmlp.c2_scale: must be [{K}] or one row per image [{nimg},{K}], got {tuple(c2_scale.shape)}")
        if (rows // nimg) % 256:
            raise _lib.FFError(f"token_projmlp: a per-image gate needs images of a multiple of 256 rows, got {rows // nimg}")
    sp = _dense(c2_scale, "token_projmlp.c2_scale", n=nimg * K, optional=True)
    gp, bp = _dense(gamma, "token_projmlp.gamma", n=K), _dense(beta, "token_projmlp.beta", n=K)
    m = pk["mlp"]
    (pwp, pbp), (wp, b1p, b2p) = _images(pk["proj"], "token_projmlp.pk.proj", "w", "b"), _images(m, "token_projmlp.pk.mlp", "w", "b1", "b2")
    nt = _nterms()
    out, op_, ldo_ = _out(None, "token_projmlp.out", tuple(x.shape), x.device)
    rows16 = (1 if att_bf16 else 0) | (2 if c2_bf16 else 0)
    if nimg > 1:
        _lib.check(_L().ff_token_projmlp_images(ap, lda, xp, ldx, cp, ldc, sp, K, nimg, rows // nimg, op_, ldo_, rows, K, m["ht"], pwp, pbp,
                                                gp, bp, float(eps), wp, b1p, b2p, nt, rows16, _stream()))
    else:
        _lib.check(_L().ff_token_projmlp(ap, lda, xp, ldx, cp, ldc, sp, op_, ldo_, rows, K, m["ht"], pwp, pbp, gp, bp, float(eps), wp, b1p,
                                         b2p, nt, rows16, _stream()))
    _note(2.0 * rows * K * K + 4.0 * rows * K * m["ht"] * 32, 4.0 * rows * K * (2 + (0.5 if att_bf16 else 1.0) + (0 if c2 is None else (0.5 if c2_bf16 else 1.0))))
    return out


@_instrument
def hab_link(att: T, x: T, pk: dict, gamma2: T, beta2: T, *, c2: T, c2_scale: T, wf: dict, rel_padded: T, gamma1: T, beta1: T,
             shift: Tuple[int, int], use_mask: bool, eps2: float = 1e-5, eps1: float = 1e-5) -> Tuple[T, T, T]:
    """One HAB's token_projmlp and the next HAB's win_attn_fused in one launch (csrc/hab_link.hip; plain bf16, 16x16 windows, six
    heads of 30): x_out = token_projmlp(att, x, pk, gamma2, beta2, c2=c2, c2_scale=c2_scale), then LayerNorm(gamma1, beta1) + qkv (wf,
    from prep.pack_win_attn) + window attention (rel_padded from prep.pack_win_rel) on x_out, which the attention takes from LDS
    instead of reading it back.  att / c2 [B,H,W,180] bf16 rows, x [B,H,W,180] fp32; c2_scale [180] (B == 1) or [B,180].
    -> (x_out fp32, xn bf16, att_out bf16), each bit-equal to the two launches."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("hab_link exists for the plain-bf16 contraction mode only")
    if c2 is None or c2_scale is None:
        raise _lib.FFError("hab_link: att and c2 must be bf16 rows, and the gate is required")
    ap, lda, B, H, W, K = _nhwc(att, "hab_link.att", dtype=_BF16)
    xp, ldx, *_ = _nhwc(x, "hab_link.x", (B, H, W, K))
    cp, ldc, *_ = _nhwc(c2, "hab_link.c2", (B, H, W, K), _BF16)
    if K != pk["mlp"]["K"] or K != wf["K"]:
        raise _lib.FFError("hab_link: shape mismatch")
    sp = _dense(c2_scale, "hab_link.c2_scale", n=B * K)
    if tuple(c2_scale.shape) not in (((K,), (1, K)) if B == 1 else ((B, K),)):
        raise _lib.FFError(f"hab_link: c2_scale must be [{K}] for one image or one row per image [{B},{K}], got {tuple(c2_scale.shape)}")
    relp = _dense(rel_padded, "hab_link.rel_padded", shape=(wf["heads"], 31, None))
    g2p, b2p_ = _dense(gamma2, "hab_link.gamma2", n=K), _dense(beta2, "hab_link.beta2", n=K)
    g1p, b1p_ = _dense(gamma1, "hab_link.gamma1", n=K), _dense(beta1, "hab_link.beta1", n=K)
    m = pk["mlp"]
    (pwp, pbp), (wp, b1p, b2p) = _images(pk["proj"], "hab_link.pk.proj", "w", "b"), _images(m, "hab_link.pk.mlp", "w", "b1", "b2")
    wfw, wfb = _images(wf, "hab_link.wf", "w", "b")
    out, op_, ldo_ = _out(None, "hab_link.out", tuple(x.shape), x.device, kind="nhwc")
    xn, xnp, ldxn = _out(None, "hab_link.xn", tuple(x.shape), x.device, bf16=True, kind="nhwc")
    ao, aop, ldao = _out(None, "hab_link.att_out", tuple(x.shape), x.device, bf16=True, kind="nhwc")
    _lib.check(_L().ff_hab_link(ap, lda, xp, ldx, cp, ldc, sp, K, B, H * W, op_, ldo_, B * H * W, K, m["ht"], pwp, pbp, g2p, b2p_, float(eps2),
                                wp, b1p, b2p, 1, 3, aop, ldao, 0, g1p, b1p_, float(eps1), wfw, wfb, relp, rel_padded.shape[1],
                                rel_padded.shape[2], H, W, 16, 16, shift[0], shift[1], int(use_mask), wf["heads"], wf["d"], xnp, ldxn, 1, 1,
                                _stream()))
    rows, nwin, nh, d = B * H * W, B * (H // 16) * (W // 16), wf["heads"], wf["d"]
    # the parents' sums (token_projmlp with bf16 att / c2, win_attn_fused with bf16 xn / out) minus the attention's read of x
    _note(2.0 * rows * K * K + 4.0 * rows * K * m["ht"] * 32 + 2.0 * nwin * 256 * K * 3 * nh * d + 4.0 * nwin * nh * 256 * 256 * d,
          4.0 * rows * K * 3.0 + 4.0 * rows * (K * 0.5 + nh * d * 0.5))
    return out, xn, ao


def cab_fused_ok(x: T) -> bool:
    """True where ops.cab_fused replaces conv2d(gelu) + conv2d(pool partials) of HAT's CAB: plain bf16, bf16 rows the kernel's 16-byte
    loads can take (a constant pitch that is a multiple of 8 elements, a 16-byte aligned base), one image of at least 1024 pixels, 180
    channels, H and W multiples of 16, and the launch within the kernel's 32-bit row offsets.  Anything else keeps the two launches."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.bfloat16 or not x.is_cuda:
        return False
    B, H, W, C = x.shape
    if not (_HALO and _GEMM_MODE == "bf16" and C == 180 and H * W >= 1024 and H % 16 == 0 and W % 16 == 0):
        return False
    try:
        xp, ld, *_ = _nhwc(x, "cab_fused.xn", dtype=_BF16)
    except _lib.FFError:                                    # no constant row pitch
        return False
    return ld % 8 == 0 and ld >= C and xp % 16 == 0 and B * H * W * max(ld, 192) < 2 ** 31


@_instrument
def cab_fused(xn: T, cab0: Tuple[T, T], cab2: Tuple[T, T], out: Optional[T] = None):
    """HAT's CAB without its gate in one launch (csrc/cab_fused.hip; plain bf16): c2 = conv3x3(gelu(conv3x3(xn) + b0)) + b2 with c1 kept in
    LDS.  xn [B,H,W,180] bf16 rows; cab0 = (packed weight [60, 9*180], bias), cab2 = (packed weight [180, 9*60], bias), the pairs conv2d
    takes.  -> (c2 bf16 rows, PoolPartials), bit for bit what conv2d(xn, *cab0, act="gelu", out_bf16=True, per_image=True) followed by
    conv2d(c1, *cab2, want_pool="partials", out_bf16=True) return: the same weight images (prep.pack_conv3x3_halo, kinds "halo1"), the
    same MFMA order, and image b's partial rows are those of its own B == 1 call."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("cab_fused exists for the plain-bf16 contraction mode only")
    from . import prep as _prep
    xp, ldi, B, H, W, Cin = _nhwc(xn, "cab_fused.xn", dtype=_BF16)
    (w0, b0), (w2, b2) = cab0, cab2
    _dense(w0, "cab_fused.w0", shape=(None, 9 * Cin))
    Cmid = w0.shape[0]
    _dense(w2, "cab_fused.w2", shape=(None, 9 * Cmid))
    Cout = w2.shape[0]
    b0p, b2p = _dense(b0, "cab_fused.b0", n=Cmid), _dense(b2, "cab_fused.b2", n=Cout)
    oshape = (B, H, W, Cout)
    if out is not None:                                     # (the caller's buffer is refused before a weight image is built)
        out, op, ldo = _out(out, "cab_fused.out", oshape, xn.device, bf16=True, kind="nhwc")
    img0 = PREPARED.get(w0, "halo1", lambda: (_prep.pack_conv3x3_halo(w0, Cin, _prep.halo_bn(Cmid), 1), _prep.halo_bn(Cmid)))
    img2 = PREPARED.get(w2, "halo1", lambda: (_prep.pack_conv3x3_halo(w2, Cmid, _prep.halo_bn(Cout), 1), _prep.halo_bn(Cout)))
    if (img0[1], img2[1]) != (64, 192):
        raise _lib.FFError(f"cab_fused: weight images of tile widths {img0[1]} / {img2[1]}, built for 64 / 192")
    i0p, i2p = _image(img0[0], "cab_fused.w0[halo1]"), _image(img2[0], "cab_fused.w2[halo1]")
    if out is None:
        out, op, ldo = _out(None, "cab_fused.out", oshape, xn.device, bf16=True, kind="nhwc")
    prow = int(_L().ff_conv3x3_halo_images_pool_rows(B, H, W, Cout, 192, 1))
    if prow < 0:
        raise _lib.FFError("cab_fused: bad shape")
    part = torch.empty((prow, 192), device=xn.device, dtype=torch.float32)
    _lib.check(_L().ff_cab_fused(xp, ldi, i0p, img0[0].numel() * img0[0].element_size(), b0p, i2p, img2[0].numel() * img2[0].element_size(),
                                 b2p, op, ldo, _dense(part, "cab_fused.part"), B, H, W, Cin, Cmid, Cout, 1, 3, _stream()))
    _note(2.0 * B * H * W * 9 * (Cin * Cmid + Cmid * Cout), 2.0 * _numel(xn, out) + 2.0 * _numel(w0, w2))
    return out, PoolPartials(part, Cout, 1.0 / float(H * W), images=B)


@_instrument
def token_linear(x: T, pk: dict, *, gamma: Optional[T] = None, beta: Optional[T] = None, eps: float = 1e-5, act=None,
                 res: Optional[T] = None, res2: Optional[T] = None, res2_scale: Optional[T] = None, want_xn: bool = False,
                 stats_range: Optional[Tuple[int, int]] = None, stats_eps: float = 1e-5):
    """res + res2*scale + act(LayerNorm?(x) @ W^T + b) for K <= 192 in one launch (bf16x3); pk from prep.pack_token_linear.
    want_xn: also return LayerNorm(x) (written by the same launch) -> (out, xn).
    stats_range=(lo, hi): also return [rows, 2] (mean, rstd) of the activated output channels [lo, hi) -> (out, stats)."""
    xp, ldx, rows, K = _rows(x, "token_linear.x")
    if K != pk["K"]:
        raise _lib.FFError("token_linear: K mismatch")
    N = pk["N"]
    rp, ldr, *_ = _rows(res, "token_linear.res", rows, N, optional=True)
    r2p, ldr2, *_ = _rows(res2, "token_linear.res2", rows, N, optional=True)
    if res2 is not None and res2_scale is None:
        raise _lib.FFError("token_linear: res2 shape mismatch")
    s2p = _dense(res2_scale, "token_linear.res2_scale", n=N, optional=True)
    if want_xn and gamma is None:
        raise _lib.FFError("token_linear: want_xn needs LayerNorm parameters")
    gp = _dense(gamma, "token_linear.gamma", n=K, optional=True)
    bp = _dense(beta, "token_linear.beta", n=K, optional=True)
    wp, wbp = _image(pk["w"], "token_linear.pk.w"), _image(pk["b"], "token_linear.pk.b", optional=True)
    nt = _nterms()
    # the padded row pitch of empty_rows makes every 32-column store segment of the kernel one whole 128-byte line (no
    # partial-line writes); consumers take the pitch as their ld argument
    out, op, ldo = _out(None, "token_linear.out", tuple(x.shape[:-1]) + (N,), x.device)
    xn, xnp, ldxn = None, None, 0
    if want_xn:
        xn, xnp, ldxn = _out(None, "token_linear.xn", tuple(x.shape), x.device)
    stats, sp, slo, shi = None, None, 0, 0
    if stats_range is not None:
        slo, shi = stats_range
        stats, sp, _ = _out(None, "token_linear.stats", (rows, 2), x.device, kind="dense")
    _lib.check(_L().ff_token_linear(xp, ldx, op, ldo, rows, K, pk["kpad"], N, pk["nt"], gp, bp, float(eps), wp, wbp, ACT[act], rp, ldr,
                                    r2p, ldr2, s2p, xnp, ldxn, sp, slo, shi, float(stats_eps), nt, _stream()))
    _note(2.0 * rows * N * K, 4.0 * (rows * K * (2 if want_xn else 1) + rows * N * (1 + (res is not None) + (res2 is not None))))
    if stats is not None:
        return out, stats
    return (out, xn) if want_xn else out


@_instrument
def token_linear_rows16(x: T, pk: dict, *, gamma: Optional[T] = None, beta: Optional[T] = None, eps: float = 1e-5,
                        out: Optional[T] = None) -> T:
    """bf16( (LayerNorm?(x) @ W^T + b) * pk["scale"] ) as bf16 rows in one launch (plain bf16 only; csrc/token_linear.hip); pk from
    prep.pack_ocab_qkv.  out (optional): a bf16 rows view [..., N] to write into."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("token_linear_rows16 exists for the plain-bf16 contraction mode only")
    xp, ldx, rows, K = _rows(x, "token_linear_rows16.x")
    if K != pk["K"]:
        raise _lib.FFError("token_linear_rows16: K mismatch")
    N = pk["N"]
    gp = _dense(gamma, "token_linear_rows16.gamma", n=K, optional=True)
    bp = _dense(beta, "token_linear_rows16.beta", n=K, optional=True)
    wp, wbp = _image(pk["w"], "token_linear_rows16.pk.w"), _image(pk["b"], "token_linear_rows16.pk.b", optional=True)
    scp = _image(pk["scale"], "token_linear_rows16.pk.scale")
    out, op, ldo = _out(out, "token_linear_rows16.out", tuple(x.shape[:-1]) + (N,), x.device, bf16=True)
    _lib.check(_L().ff_token_linear_rows16(xp, ldx, op, ldo, rows, K, pk["kpad"], N, pk["nt"], gp, bp, float(eps), wp, wbp, scp, ACT[None],
                                           None, 0, None, 0, None, None, 0, None, 0, 0, 0.0, 1, _stream()))
    _note(2.0 * rows * N * K, 4.0 * rows * K + 2.0 * rows * N)
    return out


@_instrument
def dwconv3_gate_pool(t: T, w_tap: T, bias: T):
    """t [B,H,W,2C] -> (dw3x3(t)[..., :C] * dw3x3(t)[..., C:], its per-channel mean [B,C]) in one pass.  B > 1: one launch for the
    batch (ff_dwconv3_gate_pool_images), every image with the bits of its own B == 1 call."""
    tp, ldi, B, H, W, C2 = _nhwc(t, "dwconv3_gate_pool.t")
    if B < 1 or C2 % 2:
        raise _lib.FFError("dwconv3_gate_pool: expects [B,H,W,2C] with B >= 1, [9, 2C] tap-major weights")
    wp = _dense(w_tap, "dwconv3_gate_pool.w_tap", shape=(9, C2))
    bp = _dense(bias, "dwconv3_gate_pool.bias", n=C2)
    C = C2 // 2
    out, op, _ = _out(None, "dwconv3_gate_pool.out", (B, H, W, C), t.device, kind="dense")
    pooled, pp, _ = _out(None, "dwconv3_gate_pool.pooled", (B, C), t.device, kind="dense")
    nwork = int(_L().ff_dwconv3_gate_pool_workspace(C) if B == 1 else _L().ff_dwconv3_gate_pool_images_workspace(B, C))
    work = torch.empty(nwork, device=t.device, dtype=torch.float32)
    workp = _image(work, "dwconv3_gate_pool.work")
    if B == 1:
        _lib.check(_L().ff_dwconv3_gate_pool(tp, ldi, op, C, H, W, C, wp, bp, pp, workp, nwork, _stream()))
    else:
        _lib.check(_L().ff_dwconv3_gate_pool_images(tp, ldi, op, C, B, H, W, C, wp, bp, pp, workp, nwork, _stream()))
    _note(2.0 * B * H * W * C2 * 9, 4.0 * B * H * W * (C2 + C))
    return out, pooled


@_instrument
def naf_front(x: T, pk: dict, ln_g: T, ln_b: T, w_tap: T, dw_bias: T, eps: float = 1e-6):
    """x [B,H,W,C] (C = 64 / 128) -> (SimpleGate(dw3x3(conv1(LayerNorm2d(x)))) [B,H,W,C], its per-channel mean [B,C]) in one launch;
    pk = prep.pack_token_linear(conv1 weight [2C, C], bias), w_tap [9, 2C] tap-major depth-wise weights.  B > 1: one launch for
    the batch (ff_naf_front_images), every image with the bits of its own B == 1 call."""
    xp, ldx, B, H, W, C = _nhwc(x, "naf_front.x")
    if B < 1 or C not in (64, 128) or pk["N"] != 2 * C or pk["K"] != C or pk["kpad"] != C:
        raise _lib.FFError("naf_front: expects [B,H,W,C] with B >= 1, C in (64, 128), conv1 packed as [2C, C], [9, 2C] tap-major weights")
    gp, bp = _dense(ln_g, "naf_front.ln_g", n=C), _dense(ln_b, "naf_front.ln_b", n=C)
    tapp = _dense(w_tap, "naf_front.w_tap", shape=(9, 2 * C))
    dbp = _dense(dw_bias, "naf_front.dw_bias", n=2 * C)
    wp, wbp = _image(pk["w"], "naf_front.pk.w"), _image(pk["b"], "naf_front.pk.b")
    nt = _nterms()
    out, op, _ = _out(None, "naf_front.out", (B, H, W, C), x.device, kind="dense")
    pooled, pp, _ = _out(None, "naf_front.pooled", (B, C), x.device, kind="dense")
    nwork = int(_L().ff_naf_front_workspace(H, W, C) if B == 1 else _L().ff_naf_front_images_workspace(B, H, W, C))
    work = torch.empty(nwork, device=x.device, dtype=torch.float32)
    workp = _image(work, "naf_front.work")
    if B == 1:
        _lib.check(_L().ff_naf_front(xp, ldx, H, W, C, gp, bp, float(eps), wp, wbp, tapp, dbp, op, C, pp, workp, nwork, nt, _stream()))
    else:
        _lib.check(_L().ff_naf_front_images(xp, ldx, B, H, W, C, gp, bp, float(eps), wp, wbp, tapp, dbp, op, C, pp, workp, nwork, nt,
                                            _stream()))
    _note(2.0 * B * H * W * 2 * C * (C + 9), 4.0 * B * H * W * 2 * C)
    return out, pooled


@_instrument
def naf_ffn(y: T, pk: dict, ln_g: T, ln_b: T, out_scale: T, eps: float = 1e-6, out: Optional[T] = None) -> T:
    """y + out_scale * conv5(SimpleGate(conv4(LayerNorm(y)))) in one launch (C = 64 / 128, bf16x3)."""
    yp, ldy, rows, C = _rows(y, "naf_ffn.y")
    if C != pk["C"]:
        raise _lib.FFError("naf_ffn: channel mismatch")
    gp, bp = _dense(ln_g, "naf_ffn.ln_g", n=C), _dense(ln_b, "naf_ffn.ln_b", n=C)
    sp = _dense(out_scale, "naf_ffn.out_scale", n=C)
    wp, b4p, b5p = _images(pk, "naf_ffn.pk", "w", "b4", "b5")
    nt = _nterms()
    # a fresh dense tensor of y's shape, or the caller's `out` when it is one (e.g. a leading slice of a batch's buffer)
    out, op, _ = _out(out, "naf_ffn.out", tuple(y.shape), y.device, kind="dense")
    _lib.check(_L().ff_naf_ffn(yp, ldy, op, C, rows, C, gp, bp, float(eps), wp, b4p, b5p, sp, nt, _stream()))
    _note(2.0 * rows * C * 3 * C, 8.0 * rows * C)
    return out


@_instrument
def naf_tail(g: T, x: T, pk: dict, sca: T, beta: T, ln_g: T, ln_b: T, gamma: T, eps: float = 1e-6, out: Optional[T] = None) -> T:
    """The NAFBlock tail in one launch (C = 64 / 128, plain bf16 only): y = x + beta * conv3(g * sca), then
    y + gamma * conv5(SimpleGate(conv4(LayerNorm(y)))); bit-equal to linear(g, W3, b3, res=x, mul=beta, kmul=sca) followed by
    naf_ffn.  g, x: rows views; pk from prep.pack_naf_tail.  sca [B,C] with g.shape[0] == B > 1: the rows are B equal groups, image b's
    scaled by sca[b], in one launch (ff_naf_tail_images; every image with the bits of its own call)."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError(f"naf_tail exists for the plain-bf16 contraction mode only, not {_GEMM_MODE!r}")
    gp, ldg, rows, C = _rows(g, "naf_tail.g", C=pk["C"])
    xp, ldx, *_ = _rows(x, "naf_tail.x", rows, C)
    if tuple(x.shape) != tuple(g.shape):
        raise _lib.FFError("naf_tail: shape mismatch")
    images = sca.shape[0] if isinstance(sca, torch.Tensor) and sca.dim() == 2 and sca.shape[0] > 1 else 1
    if images > 1 and (g.dim() < 2 or g.shape[0] != images):
        raise _lib.FFError(f"naf_tail: sca {tuple(sca.shape)} must be a contiguous [B, {C}] matrix with B the leading dimension of g {tuple(g.shape)}")
    scap = _dense(sca, "naf_tail.sca", shape=(images, C)) if images > 1 else _dense(sca, "naf_tail.sca", n=C)
    bep, gap = _dense(beta, "naf_tail.beta", n=C), _dense(gamma, "naf_tail.gamma", n=C)
    lgp, lbp = _dense(ln_g, "naf_tail.ln_g", n=C), _dense(ln_b, "naf_tail.ln_b", n=C)
    wp, b3p, b4p, b5p = _images(pk, "naf_tail.pk", "w", "b3", "b4", "b5")
    out, op, _ = _out(out, "naf_tail.out", tuple(x.shape), x.device, kind="dense")
    if images > 1:
        _lib.check(_L().ff_naf_tail_images(gp, ldg, xp, ldx, op, C, rows, C, scap, images, rows // images, b3p, bep, lgp, lbp, float(eps),
                                           wp, b4p, b5p, gap, _stream()))
    else:
        _lib.check(_L().ff_naf_tail(gp, ldg, xp, ldx, op, C, rows, C, scap, b3p, bep, lgp, lbp, float(eps), wp, b4p, b5p, gap, _stream()))
    _note(2.0 * rows * C * 4 * C, 12.0 * rows * C)
    return out


@_instrument
def layernorm(x: T, gamma: T, beta: T, eps: float = 1e-5, out: Optional[T] = None, out_bf16: bool = False) -> T:
    """out_bf16: bf16 output rows, (bf16) of the fp32 result, for a consumer that rounds them to bf16 anyway."""
    xp, ldi, rows, C = _rows(x, "layernorm.x")
    if out is not None and (out.dtype == torch.bfloat16) != out_bf16:
        raise _lib.FFError("layernorm: out dtype does not match out_bf16")
    gp, bp = _dense(gamma, "layernorm.gamma", n=C), _dense(beta, "layernorm.beta", n=C)
    out, op, ldo = _out(out, "layernorm.out", tuple(x.shape), x.device, bf16=out_bf16)
    fn = _L().ff_layernorm_bf16out if out_bf16 else _L().ff_layernorm
    _lib.check(fn(xp, ldi, op, ldo, rows, C, gp, bp, float(eps), _stream()))
    _note(0.0, (6.0 if out_bf16 else 8.0) * rows * C)
    return out


def pool_partials(x: T):
    """First stage of the global average pool of x [B,H,W,C] -> PoolPartials (vec_mlp finishes them in its own launch).  B > 1: one
    launch for the batch (ff_pool_partials_images; H * W a multiple of 256), PoolPartials(images=B) holding image b's rows as its own
    B == 1 call writes them."""
    xp, ld, B, H, W, C = _nhwc(x, "pool_partials.x")
    P = H * W
    if B != 1 and (B < 1 or P % 256):
        raise _lib.FFError(f"pool_partials: a batch needs images of a multiple of 256 pixels, got {tuple(x.shape)}")
    rows = int(_L().ff_pool_partial_rows(P) if B == 1 else _L().ff_pool_partials_images_rows(B, P))
    part, pp, _ = _out(None, "pool_partials.part", (rows, C), x.device, kind="dense")
    if B == 1:
        _lib.check(_L().ff_pool_partials(xp, ld, P, C, pp, part.numel(), _stream()))
    else:
        _lib.check(_L().ff_pool_partials_images(xp, ld, B, P, C, pp, part.numel(), _stream()))
    return PoolPartials(part, C, 1.0 / float(P), images=B)


@_instrument
def pool_mean(x: T) -> T:
    """[B,H,W,C] rows view -> [B,C]."""
    xp, ld, B, H, W, C = _nhwc(x, "pool_mean.x")
    P = H * W
    nwork = int(_L().ff_pool_mean_workspace(B, P, C))
    work = torch.empty(nwork, device=x.device, dtype=torch.float32)
    out, op, _ = _out(None, "pool_mean.out", (B, C), x.device, kind="dense")
    _lib.check(_L().ff_pool_mean(xp, ld, B, P, C, op, _image(work, "pool_mean.work"), nwork, _stream()))
    _note(0.0, 4.0 * B * P * C)
    return out


@_instrument
def vec_mlp(v, W1: T, b1: Optional[T], act1, W2: Optional[T] = None, b2: Optional[T] = None, act2=None,
            post: float = 1.0) -> T:
    """act2(W2 . act1(W1 . v + b1) + b2) * post per row of v [B, Cin] (W2 None: one layer).  v may be a PoolPartials: the pool is
    then finished inside the same launch (two-layer form with a hidden width <= 64), otherwise finished first."""
    vp = None if isinstance(v, PoolPartials) else _dense(v, "vec_mlp.v", shape=(None, None))
    for t_, n_ in ((W1, "W1"),) + (() if W2 is None else ((W2, "W2"),)):
        _dev(t_, "vec_mlp." + n_, _F32)
        if t_.dim() < 2:
            raise _lib.FFError(f"vec_mlp.{n_}: expected a [out, in] matrix, got {tuple(t_.shape)}")
    Ch = W1.shape[0]
    fused = vp is None and W2 is not None and Ch <= 64 and v.C <= 512
    Cin = v.C if vp is None else v.shape[1]
    Cout = W2.shape[0] if W2 is not None else Ch
    if W1.shape[1] != Cin or (W2 is not None and W2.shape[1] != Ch):
        raise _lib.FFError("vec_mlp: weight shape mismatch")
    w1p, b1p = _dense(W1, "vec_mlp.W1", n=Ch * Cin), _dense(b1, "vec_mlp.b1", n=Ch, optional=True)
    w2p, b2p = _dense(W2, "vec_mlp.W2", n=Cout * Ch, optional=True), _dense(b2, "vec_mlp.b2", n=Cout, optional=True)
    if fused:
        vp = _dense(v.part, "vec_mlp.v.part", shape=(v.images * v.rows_per_image, None))
        out, op, _ = _out(None, "vec_mlp.out", (v.images, Cout), v.part.device, kind="dense")
        if v.images > 1:                                 # one workgroup per image, each in the single-image summation order
            _lib.check(_L().ff_pool_vec_mlp_images(vp, v.images, v.rows_per_image, v.part.shape[1], v.inv_count, v.C, w1p, b1p, Ch,
                                                   ACT[act1], w2p, b2p, Cout, ACT[act2], float(post), op, None, _stream()))
        else:
            _lib.check(_L().ff_pool_vec_mlp(vp, v.part.shape[0], v.part.shape[1], v.inv_count, v.C, w1p, b1p, Ch, ACT[act1], w2p, b2p,
                                            Cout, ACT[act2], float(post), op, None, _stream()))
        return out
    if vp is None:
        v = v.mean()
        vp = _dense(v, "vec_mlp.v", shape=(None, Cin))
    B = v.shape[0]
    out, op, _ = _out(None, "vec_mlp.out", (B, Cout), v.device, kind="dense")
    _lib.check(_L().ff_vec_mlp(vp, B, Cin, w1p, b1p, Ch, ACT[act1], w2p, b2p, Cout, ACT[act2], float(post), op, _stream()))
    return out


@_instrument
def pixel_mlp(x: T, W1: T, b1: Optional[T], act1, w2: T, b2: float, act2) -> T:
    """[..., C] rows -> [..., 1]: act2(w2 . act1(W1 x + b1) + b2) per row, hidden width <= 16 (fp32, one launch)."""
    xp, ldi, rows, C = _rows(x, "pixel_mlp.x")
    w1p = _dense(W1, "pixel_mlp.W1", shape=(None, C))
    Hd = W1.shape[0]
    b1p = _dense(b1, "pixel_mlp.b1", n=Hd, optional=True)
    _dev(w2, "pixel_mlp.w2", _F32)
    w2p = _dense(w2.reshape(-1), "pixel_mlp.w2", n=Hd)
    out, op, _ = _out(None, "pixel_mlp.out", tuple(x.shape[:-1]) + (1,), x.device, kind="dense")
    _lib.check(_L().ff_pixel_mlp(xp, ldi, rows, C, Hd, w1p, b1p, ACT[act1], w2p, float(b2), ACT[act2], op, _stream()))
    _note(2.0 * rows * C * Hd, 4.0 * rows * (C + 1))
    return out


@_instrument
def dwconv2d(x: T, w_tap: T, bias: Optional[T] = None, *, ksize=(3, 3), stride=(1, 1), pad=(1, 1),
             post_scale: Optional[T] = None, post_shift: Optional[T] = None, act=None, out: Optional[T] = None,
             mul_in: Optional[T] = None) -> T:
    xp, ldi, B, H, W, C = _nhwc(x, "dwconv2d.x")
    KH, KW = ksize
    wp = _dense(w_tap, "dwconv2d.w_tap", shape=(KH * KW, C))
    Ho = (H + 2 * pad[0] - KH) // stride[0] + 1
    Wo = (W + 2 * pad[1] - KW) // stride[1] + 1
    bp = _dense(bias, "dwconv2d.bias", n=C, optional=True)
    psp = _dense(post_scale, "dwconv2d.post_scale", n=C, optional=True)
    php = _dense(post_shift, "dwconv2d.post_shift", n=C, optional=True)
    if out is None:
        out, op, ldo = _out(None, "dwconv2d.out", (B, Ho, Wo, C), x.device, kind="nhwc")
    else:                                                    # the caller's buffer: any NHWC rows view, as before
        op, ldo, *_ = _nhwc(out, "dwconv2d.out")
    mp, ldm, *_ = _nhwc(mul_in, "dwconv2d.mul_in", (B, Ho, Wo, C), optional=True)
    _lib.check(_L().ff_dwconv2d(xp, ldi, op, ldo, B, H, W, C, Ho, Wo, wp, bp, KH, KW, stride[0], stride[1], pad[0], pad[1], psp, php,
                                ACT[act], mp, ldm, _stream()))
    _note(2.0 * B * Ho * Wo * C * KH * KW, 4.0 * (B * H * W * C + B * Ho * Wo * C))
    return out


@_instrument
def token_linear_gated(x: T, x2: T, pk: dict, cm: T, gb2: float, *, res: Optional[T] = None) -> T:
    """res + W (x * cm[channel] + x2 * sm[token]) + b with sm = sigmoid(gw2 . gelu(GW1 x + gb1) + gb2) in one launch (bf16x3);
    pk from prep.pack_token_linear_gated.  cm [K] (or [1,K]): one channel gate for every row.  cm [B,K] with B > 1: the rows are B images of
    a multiple of 256 rows each, image b gated by cm[b], in one launch (ff_token_linear_gated_images) -- bit-equal to B calls."""
    xp, ldx, rows, K = _rows(x, "token_linear_gated.x", C=pk["K"])
    x2p, ldx2, *_ = _rows(x2, "token_linear_gated.x2", rows, K)
    _dev(cm, "token_linear_gated.cm", _F32)
    images = 1
    if cm.numel() != K:                                      # (refusals first: nothing is launched before them)
        if cm.dim() != 2 or cm.shape[1] != K or cm.shape[0] < 1 or not cm.is_contiguous():
            raise _lib.FFError(f"token_linear_gated: cm must be [{K}] or one contiguous row per image [B,{K}], got {tuple(cm.shape)}")
        images = int(cm.shape[0])
        if rows % images or (rows // images) % 256:
            raise _lib.FFError(f"token_linear_gated: a per-image gate needs B = {images} images of a multiple of 256 rows, got {rows} rows")
    cmp_ = _dense(cm, "token_linear_gated.cm", n=images * K)
    N = pk["N"]
    rp, ldr, *_ = _rows(res, "token_linear_gated.res", rows, N, optional=True)
    gb1p, gw2p, wp, wbp = _images(pk, "token_linear_gated.pk", "gb1", "gw2", "w", "b")
    nt = _nterms()
    out, op, ldo = _out(None, "token_linear_gated.out", tuple(x.shape[:-1]) + (N,), x.device)
    if images > 1:
        _lib.check(_L().ff_token_linear_gated_images(xp, ldx, x2p, ldx2, cmp_, images, rows // images, gb1p, gw2p, float(gb2), op, ldo,
                                                     rows, K, N, pk["nt"], wp, wbp, rp, ldr, nt, _stream()))
    else:
        _lib.check(_L().ff_token_linear_gated(xp, ldx, x2p, ldx2, cmp_, None, gb1p, gw2p, float(gb2), op, ldo, rows, K, N, pk["nt"], wp,
                                              wbp, rp, ldr, nt, _stream()))
    _note(2.0 * rows * N * K + 2.0 * rows * 32 * K, 4.0 * rows * (2 * K + N * (2 if res is not None else 1)))
    return out


@_instrument
def dwconv3x3_ln(x: T, w_tap: T, bias: Optional[T], stats: T, gamma: T, beta: T, mul_in: Optional[T] = None) -> T:
    """(dw3x3(LayerNorm(x)) + bias) * mul_in with the LayerNorm applied on load from per-token (mean, rstd) `stats`."""
    xp, ldi, B, H, W, C = _nhwc(x, "dwconv3x3_ln.x")
    wp = _dense(w_tap, "dwconv3x3_ln.w_tap", shape=(9, C))
    bp = _dense(bias, "dwconv3x3_ln.bias", n=C, optional=True)
    sp = _dense(stats, "dwconv3x3_ln.stats", shape=(B * H * W, 2))
    gp, bep = _dense(gamma, "dwconv3x3_ln.gamma", n=C), _dense(beta, "dwconv3x3_ln.beta", n=C)
    out, op, ldo = _out(None, "dwconv3x3_ln.out", (B, H, W, C), x.device, kind="nhwc")
    mp, ldm, *_ = _nhwc(mul_in, "dwconv3x3_ln.mul_in", (B, H, W, C), optional=True)
    _lib.check(_L().ff_dwconv3x3_ln(xp, ldi, op, ldo, B, H, W, C, wp, bp, sp, gp, bep, mp, ldm, _stream()))
    _note(2.0 * B * H * W * C * 9, 4.0 * B * H * W * C * (3 if mul_in is not None else 2))
    return out


@_instrument
def sgfn_tail(y: T, c2: int, w_tap: T, dw_bias: Optional[T], stats: T, gamma: T, beta: T, w2: T, b2: Optional[T], res: Optional[T] = None) -> T:
    """res + fc2(y[..., :c2] * (dw3x3(LayerNorm(y[..., c2:2 c2])) + dw_bias)) + b2 in one launch (plain bf16; csrc/sgfn_tail.hip).
    y [B,H,W,>= 2 c2] rows view (fc1's output), stats [B*H*W, 2] = (mean, rstd) of y[..., c2:], w_tap [9, c2], w2 [N, c2]."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("sgfn_tail exists for the plain-bf16 contraction mode only")
    yp, ldh, B, H, W, Cy = _nhwc(y, "sgfn_tail.y")
    _dev(w2, "sgfn_tail.w2", _F32)
    if w2.dim() != 2 or w2.shape[1] != c2:
        raise _lib.FFError(f"sgfn_tail.w2: expected [N, {c2}], got {tuple(w2.shape)}")
    N = w2.shape[0]
    if Cy < 2 * c2:
        raise _lib.FFError("sgfn_tail: shape mismatch")
    tapp = _dense(w_tap, "sgfn_tail.w_tap", shape=(9, c2))
    dbp = _dense(dw_bias, "sgfn_tail.dw_bias", n=c2, optional=True)
    sp = _dense(stats, "sgfn_tail.stats", shape=(B * H * W, 2))
    gp, bep = _dense(gamma, "sgfn_tail.gamma", n=c2), _dense(beta, "sgfn_tail.beta", n=c2)
    b2p = _dense(b2, "sgfn_tail.b2", n=N, optional=True)
    rp, ldr, *_ = _nhwc(res, "sgfn_tail.res", (B, H, W, N), optional=True)
    from . import prep as _prep
    tiles = PREPARED.get(w2, "sgfn", lambda: _prep.pack_sgfn_fc2(w2))
    out, op, ldo = _out(None, "sgfn_tail.out", (B, H, W, N), y.device, kind="nhwc")
    _lib.check(_L().ff_sgfn_tail(yp, ldh, c2, sp, gp, bep, tapp, dbp, _image(tiles, "sgfn_tail.w2[sgfn]"), tiles.shape[0], b2p, rp, ldr,
                                 op, ldo, B, H, W, N, _stream()))
    _note(2.0 * B * H * W * c2 * (9 + N), 4.0 * B * H * W * (2 * c2 + 2 * N))
    return out


@_instrument
def mix2(a: T, b: Optional[T] = None, *, ka: float = 1.0, kb: float = 1.0, ca: Optional[T] = None,
         cb: Optional[T] = None, pa: Optional[T] = None, pb: Optional[T] = None, clamp01: bool = False,
         out: Optional[T] = None) -> T:
    """out = ka*a*ca[c]*pa[p] + kb*b*cb[c]*pb[p].  ca [B, C] with B > 1: the rows are B equal groups (one image each) and group b is scaled
    by ca[b], in one launch (ff_mix2_images) -- every image with the bits of its own call with ca[b]."""
    ap, lda, rows, C = _rows(a, "mix2.a")
    bp, ldb, *_ = _rows(b, "mix2.b", rows, C, optional=True)
    out, op, ldo = _out(out, "mix2.out", tuple(a.shape), a.device)
    pap, ldpa, *_ = _rows(pa, "mix2.pa", rows, 1, optional=True)     # per-row vectors [rows, 1]
    pbp, ldpb, *_ = _rows(pb, "mix2.pb", rows, 1, optional=True)
    images = 1
    if isinstance(ca, torch.Tensor) and ca.dim() == 2 and ca.shape[0] > 1:
        images = int(ca.shape[0])
        if ca.shape[1] != C or rows % images:
            raise _lib.FFError(f"mix2: ca {tuple(ca.shape)} must be a contiguous [B, {C}] matrix with B dividing the {rows} rows")
    cap = _dense(ca, "mix2.ca", n=C * images, optional=True)
    cbp = _dense(cb, "mix2.cb", n=C, optional=True)
    if images > 1:
        _lib.check(_L().ff_mix2_images(op, ldo, ap, lda, bp, ldb, rows, C, float(ka), float(kb), cap, images, rows // images,
                                       cbp, pap, ldpa, pbp, ldpb, int(clamp01), _stream()))
    else:
        _lib.check(_L().ff_mix2(op, ldo, ap, lda, bp, ldb, rows, C, float(ka), float(kb), cap, cbp, pap, ldpa, pbp, ldpb, int(clamp01),
                                _stream()))
    _note(0.0, 4.0 * rows * C * (3 if b is not None else 2))
    return out


@_instrument
def fma3(a: Optional[T], b: T, c: T, alpha: float = 1.0, out: Optional[T] = None) -> T:
    bp, ldb, rows, C = _rows(b, "fma3.b")
    cp, ldc, *_ = _rows(c, "fma3.c", rows, C)
    ap, lda, *_ = _rows(a, "fma3.a", rows, C, optional=True)
    out, op, ldo = _out(out, "fma3.out", tuple(b.shape), b.device)
    _lib.check(_L().ff_fma3(op, ldo, ap, lda, bp, ldb, cp, ldc, rows, C, float(alpha), _stream()))
    _note(0.0, 4.0 * rows * C * (4 if a is not None else 3))
    return out


@_instrument
def affine(x: T, scale: T, shift: T, act=None, out: Optional[T] = None) -> T:
    xp, ldi, rows, C = _rows(x, "affine.x")
    scp, shp = _dense(scale, "affine.scale", n=C), _dense(shift, "affine.shift", n=C)
    out, op, ldo = _out(out, "affine.out", tuple(x.shape), x.device)
    _lib.check(_L().ff_affine(op, ldo, xp, ldi, rows, C, scp, shp, ACT[act], _stream()))
    _note(0.0, 8.0 * rows * C)
    return out


def u8_to_f32_image(img_u8: T) -> T:
    """uint8 HWC [H,W,3] on the device -> fp32 [1,3,H,W] in [0,1] (reference io.py:64-68)."""
    ip = _dense(img_u8, "u8_to_f32_image.img_u8", _U8, shape=(None, None, 3))
    H, W, _ = img_u8.shape
    out, op, _ = _out(None, "u8_to_f32_image.out", (1, 3, H, W), img_u8.device, kind="dense")
    _lib.check(_L().ff_u8hwc_to_f32nchw(ip, op, H, W, _stream()))
    return out


def f32_to_u8_image(x: T) -> T:
    """fp32 [1,3,H,W] (or [3,H,W]) -> uint8 HWC [H,W,3]: clamp, *255, round half to even (reference io.py:71-76)."""
    _dev(x, "f32_to_u8_image.x", _F32)
    if x.dim() == 4:
        if x.shape[0] != 1:
            raise _lib.FFError("f32_to_u8_image: batch must be 1")
        x = x[0]
    if x.dim() != 3 or x.shape[0] != 3:
        raise _lib.FFError("f32_to_u8_image: expected [1,3,H,W] or [3,H,W]")
    x = x.contiguous()
    _, H, W = x.shape
    out = torch.empty((H, W, 3), device=x.device, dtype=torch.uint8)
    _lib.check(_L().ff_f32nchw_to_u8hwc(_dense(x, "f32_to_u8_image.x"), _dense(out, "f32_to_u8_image.out", _U8), H, W, _stream()))
    return out


@_instrument
def nchw_to_nhwc(x: T, Hp: Optional[int] = None, Wp: Optional[int] = None, add: Optional[T] = None,
                 pad_mode: str = "zero", out: Optional[T] = None) -> T:
    _dev(x, "nchw_to_nhwc.x", _F32)
    x = x.contiguous()
    xp = _dense(x, "nchw_to_nhwc.x", shape=(None, None, None, None))
    B, C, H, W = x.shape
    Hp, Wp = Hp or H, Wp or W
    addp = _dense(add, "nchw_to_nhwc.add", n=C, optional=True)
    if out is None:
        out = empty_rows((B, Hp, Wp, C), x.device)
    op, ldo, *_ = _nhwc(out, "nchw_to_nhwc.out")             # the caller's buffer: any NHWC rows view, as before
    _lib.check(_L().ff_nchw_to_nhwc(xp, op, B, C, H, W, Hp, Wp, ldo, addp, 1 if pad_mode == "reflect" else 0,
                                    _stream()))
    return out


@_instrument
def nhwc_to_nchw(x: T, H: Optional[int] = None, W: Optional[int] = None, add: Optional[T] = None, clamp01: bool = False,
                 out: Optional[T] = None) -> T:
    xp, ldi, B, Hs, Ws, C = _nhwc(x, "nhwc_to_nchw.x")
    H, W = H or Hs, W or Ws
    addp = _dense(add, "nhwc_to_nchw.add", n=C, optional=True)
    out, op, _ = _out(out, "nhwc_to_nchw.out", (B, C, H, W), x.device, kind="dense")
    _lib.check(_L().ff_nhwc_to_nchw(xp, op, B, C, H, W, Hs, Ws, ldi, addp, int(clamp01), _stream()))
    return out


def _aten_scale(n_in: int, n_out: int, scale_factor: Optional[float]) -> float:
    """ATen area_pixel_compute_scale (align_corners=False): 1/scale_factor if given else in/out, in fp32."""
    import numpy as np
    if scale_factor is not None and scale_factor > 0:
        return float(np.float32(1.0) / np.float32(scale_factor))
    return float(np.float32(n_in) / np.float32(n_out))


@_instrument
def resize(x: T, size: Tuple[int, int], *, mode: str = "bilinear", scale_factor: Optional[float] = None,
           layout: str = "nhwc", out: Optional[T] = None, mul: float = 1.0) -> T:
    """x NHWC rows view [B,H,W,C] or planar [B,C,H,W] (layout='nchw'); out is always NHWC (may be a channel slice)."""
    Ho, Wo = size
    if layout == "nhwc":
        xp, ld, B, Hi, Wi, C = _nhwc(x, "resize.x")
        isb, isc, isy, isx = Hi * Wi * ld, 1, Wi * ld, ld
    else:
        _dev(x, "resize.x", _F32)
        x = x.contiguous()
        xp = _dense(x, "resize.x", shape=(None, None, None, None))
        B, C, Hi, Wi = x.shape
        isb, isc, isy, isx = C * Hi * Wi, Hi * Wi, Wi, 1
    if out is None:
        out = torch.empty((B, Ho, Wo, C), device=x.device, dtype=torch.float32)
    op, ldo, _, oh, ow, _ = _nhwc(out, "resize.out", (B, None, None, C))   # out may be larger than (Ho, Wo): the top-left region is written
    if oh < Ho or ow < Wo:
        raise _lib.FFError("resize: out shape mismatch")
    sh = _aten_scale(Hi, Ho, scale_factor)
    sw = _aten_scale(Wi, Wo, scale_factor)
    _lib.check(_L().ff_resize(xp, isb, isc, isy, isx, Hi, Wi, op, oh * ow * ldo, 1, ow * ldo, ldo, Ho, Wo, B, C, sh, sw,
                              0 if mode == "bilinear" else 1, float(mul), _stream()))
    _note(0.0, 4.0 * B * C * (Hi * Wi + Ho * Wo))
    return out


@_instrument
def avgpool2(x: T) -> T:
    xp, ldi, B, H, W, C = _nhwc(x, "avgpool2.x")
    out, op, _ = _out(None, "avgpool2.out", (B, H // 2, W // 2, C), x.device, kind="dense")
    _lib.check(_L().ff_avgpool2(xp, ldi, op, C, B, H, W, C, _stream()))
    return out


def _planar_images(x: T, out: T, name: str):
    """Planar image(s) [3,H,W] or contiguous [B,3,H,W] and their NHWC output [B,H,W,>=..] -> (x pointer, B, C, H, W, out pointer, ldo)."""
    xp = _dense(x, name + ".x")
    B = int(x.shape[0]) if x.dim() == 4 else 1
    C, H, W = x.shape[-3:]
    op, ldo, ob, oh, ow, _ = _nhwc(out, name + ".out")
    if B > 1 and (C != 3 or (ob, oh, ow) != (B, H, W)):
        raise _lib.FFError(f"{name}: expected contiguous planar images [B,3,H,W] and out [B,H,W,.], got {tuple(x.shape)} and {tuple(out.shape)}")
    if B > 1 and out.stride(0) != H * W * ldo:
        raise _lib.FFError(f"{name}: the images of out must follow each other ([B,H,W,ld] rows)")
    return xp, B, C, H, W, op, ldo


@_instrument
def dct8_bands(x_planar: T, dct_mat: T, masks3: T, band_scale: T, out: T, ch_off: int):
    """x_planar [3,H,W] (or [1,3,H,W]); [B,3,H,W] with B > 1: the batch in one launch (ff_dct8_bands_images)."""
    xp, B, C, H, W, op, ldo = _planar_images(x_planar, out, "dct8_bands")
    dp, mp = _dense(dct_mat, "dct8_bands.dct_mat", n=64), _dense(masks3, "dct8_bands.masks3", n=3 * 64)
    sp = _dense(band_scale, "dct8_bands.band_scale", n=3)
    if B > 1:
        _lib.check(_L().ff_dct8_bands_images(xp, B, H, W, dp, mp, sp, op, ldo, ch_off, _stream()))
    else:
        _lib.check(_L().ff_dct8_bands(xp, C, H, W, dp, mp, sp, op, ldo, ch_off, _stream()))


@_instrument
def dwt_pass(x_planar: T, axis: int, lo8: T, hi8: T) -> Tuple[T, T]:
    xp = _dense(x_planar, "dwt_pass.x", shape=(None, None, None))
    C, H, W = x_planar.shape
    lp, hp = _dense(lo8, "dwt_pass.lo8", n=8), _dense(hi8, "dwt_pass.hi8", n=8)
    Ho = (H + 6) // 2 + 1 if axis == 0 else H
    Wo = (W + 6) // 2 + 1 if axis == 1 else W
    lo = torch.empty((C, Ho, Wo), device=x_planar.device, dtype=torch.float32)
    hi = torch.empty_like(lo)
    _lib.check(_L().ff_dwt_pass(xp, C, H, W, axis, lp, hp, _dense(lo, "dwt_pass.lo"), _dense(hi, "dwt_pass.hi"), _stream()))
    return lo, hi


@_instrument
def fft_bands(x_planar: T, twW: Tuple[T, T], twH: Tuple[T, T], mask_logits: T, temp: float, band_scale2: T, out: T,
              ch_lo: int, ch_hi: int):
    xp, B, C, H, W, op, ldo = _planar_images(x_planar, out, "fft_bands")
    _dev(mask_logits, "fft_bands.mask_logits", _F32)
    msz = mask_logits.shape[-1]
    tw = (_dense(twW[0], "fft_bands.twW[0]", n=W), _dense(twW[1], "fft_bands.twW[1]", n=W),
          _dense(twH[0], "fft_bands.twH[0]", n=H), _dense(twH[1], "fft_bands.twH[1]", n=H))
    mp = _dense(mask_logits, "fft_bands.mask_logits", n=msz * msz)
    sp = _dense(band_scale2, "fft_bands.band_scale2", n=2)
    if B > 1:                                                # the batch through one run of the four kernels (ff_fft_bands_images)
        nwork = int(_L().ff_fft_bands_images_workspace(B, H, W))
        if nwork < 0:
            raise _lib.FFError(f"fft_bands: no batched form for {tuple(x_planar.shape)}")
    else:
        nwork = 4 * C * H * (W // 2 + 1)
    work = torch.empty(nwork, device=x_planar.device, dtype=torch.float32)
    workp = _image(work, "fft_bands.work")
    if B > 1:
        _lib.check(_L().ff_fft_bands_images(xp, B, H, W, *tw, mp, msz, float(temp), sp, workp, nwork, op, ldo, ch_lo, ch_hi, _stream()))
    else:
        _lib.check(_L().ff_fft_bands(xp, C, H, W, *tw, mp, msz, float(temp), sp, workp, nwork, op, ldo, ch_lo, ch_hi, _stream()))


@_instrument
def chan_attn_weights(qkv: T, q_off: int, k_off: int, temperature: T) -> T:
    qp, ld, rows, C = _rows(qkv, "chan_attn_weights.qkv")
    tp = _dense(temperature, "chan_attn_weights.temperature", n=6)      # one per head: six heads of 30 channels
    nwork = int(_L().ff_chan_attn_workspace(rows))
    work = torch.empty(nwork, device=qkv.device, dtype=torch.float32)
    wbd, wbdp, _ = _out(None, "chan_attn_weights.wbd", (180, 180), qkv.device, kind="dense")
    _lib.check(_L().ff_chan_attn_weights(qp, ld, q_off, k_off, rows, tp, wbdp, _image(work, "chan_attn_weights.work"), nwork, _stream()))
    return wbd


@_instrument
def chan_qkv_attn(x: T, pk: dict, gamma: T, beta: T, temperature: T, eps: float = 1e-5):
    """DAT channel attention front end in two launches (ff_chan_qkv + ff_chan_attn_finish): x [..., 180] ->
    (v [..., 180], block-diagonal attention matrix [180, 180]); q and k never reach memory.
    x [B,H,W,180] with B > 1 (H * W a multiple of 256): still two launches -- ff_chan_qkv's partials are per 256-token workgroup, so one call
    covers the batch, and ff_chan_attn_finish_images reduces every image's own blocks in the single-image order -> wbd [B,180,180], every
    image's matrix (and v) with the bits of its own call."""
    xp, ldx, rows, K = _rows(x, "chan_qkv_attn.x")
    if K != pk["K"]:
        raise _lib.FFError("chan_qkv_attn: K mismatch")
    images = int(x.shape[0]) if x.dim() == 4 and x.shape[0] > 1 else 1
    if images > 1 and (rows // images) % 256:
        raise _lib.FFError(f"chan_qkv_attn: a batch needs images of a multiple of 256 tokens, got {tuple(x.shape)}")
    gp, bp = _dense(gamma, "chan_qkv_attn.gamma", n=K), _dense(beta, "chan_qkv_attn.beta", n=K)
    tp = _dense(temperature, "chan_qkv_attn.temperature", n=6)          # one per head: six heads of 30 channels
    wp, wbp = _image(pk["w"], "chan_qkv_attn.pk.w"), _image(pk["b"], "chan_qkv_attn.pk.b")
    nt = _nterms()
    v, vp, ldv = _out(None, "chan_qkv_attn.v", tuple(x.shape), x.device)
    nwork = int(_L().ff_chan_qkv_images_workspace(images, rows // images)) if images > 1 else int(_L().ff_chan_qkv_workspace(rows))
    work = torch.empty(nwork, device=x.device, dtype=torch.float32)
    workp = _image(work, "chan_qkv_attn.work")
    wbd, wbdp, _ = _out(None, "chan_qkv_attn.wbd", (images, 180, 180) if images > 1 else (180, 180), x.device, kind="dense")
    _lib.check(_L().ff_chan_qkv(xp, ldx, rows, K, gp, bp, float(eps), wp, wbp, vp, ldv, workp, nwork, nt, _stream()))
    if images > 1:
        _lib.check(_L().ff_chan_attn_finish_images(workp, nwork, images, rows // images, tp, wbdp, _stream()))
    else:
        _lib.check(_L().ff_chan_attn_finish(workp, nwork, (rows + 255) // 256, tp, wbdp, _stream()))
    _note(2.0 * rows * 576 * K + 2.0 * rows * 6 * 32 * 32, 8.0 * rows * K)
    return v, wbd


@_instrument
def band_mha_core(qkv: T, P: int, nbands: int, heads: int) -> T:
    _dev(qkv, "band_mha_core.qkv", _F32)
    E = qkv.shape[-1] // 3
    qp = _dense(qkv, "band_mha_core.qkv", n=P * nbands * 3 * E)
    out, op, _ = _out(None, "band_mha_core.out", (P * nbands, E), qkv.device, kind="dense")
    _lib.check(_L().ff_band_mha_core(qp, op, P, nbands, heads, _stream()))
    return out


@_instrument
def band_weight(x: T, att: T, imp: T) -> T:
    xp = _dense(x, "band_weight.x")
    nb = x.shape[-1] // 3
    P = x.numel() // x.shape[-1]
    ap, ip = _dense(att, "band_weight.att", n=P * nb), _dense(imp, "band_weight.imp", n=nb)
    out = torch.empty_like(x)
    _lib.check(_L().ff_band_weight(xp, ap, ip, _dense(out, "band_weight.out"), P, nb, _stream()))
    return out


@_instrument
def freq_guidance(b3: T) -> T:
    bp = _dense(b3, "freq_guidance.b3")
    P = b3.numel() // 9
    out, op, _ = _out(None, "freq_guidance.out", tuple(b3.shape[:-1]) + (3,), b3.device, kind="dense")
    _lib.check(_L().ff_freq_guidance(bp, op, P, _stream()))
    return out


@_instrument
def dynamic_gates(graw: T, dif: T) -> T:
    gp = _dense(graw, "dynamic_gates.graw")
    P = graw.numel() // 3
    dp = _dense(dif, "dynamic_gates.dif", n=P)
    out = torch.empty_like(graw)
    _lib.check(_L().ff_dynamic_gates(gp, dp, _dense(out, "dynamic_gates.out"), P, _stream()))
    return out


@_instrument
def fuse_blend(experts9: T, hier3: T, guide3: T, gates3: T, dif1: T) -> T:
    """experts9 [B,Hh,Wh,9], hier3 [B,Hh,Wh,3], guide3 / gates3 [B,Hl,Wl,3], dif1 [B,Hl,Wl,1], all contiguous -> [B,Hh,Wh,3]; B > 1 in one
    launch (ff_fuse_blend_images)."""
    ep = _dense(experts9, "fuse_blend.experts9", shape=(None, None, None, 9))
    B, Hh, Wh, _ = experts9.shape
    gp = _dense(guide3, "fuse_blend.guide3", shape=(B, None, None, 3))
    _, Hl, Wl, _ = guide3.shape
    hp, tp = _dense(hier3, "fuse_blend.hier3", shape=(B, Hh, Wh, 3)), _dense(gates3, "fuse_blend.gates3", shape=(B, Hl, Wl, 3))
    dp = _dense(dif1, "fuse_blend.dif1", n=B * Hl * Wl)
    out, op, _ = _out(None, "fuse_blend.out", (B, Hh, Wh, 3), experts9.device, kind="dense")
    if B > 1:
        if tuple(dif1.shape) != (B, Hl, Wl, 1):
            raise _lib.FFError(f"fuse_blend: a batch needs contiguous [{B},{Hl},{Wl},1] tensors, got {tuple(dif1.shape)}")
        _lib.check(_L().ff_fuse_blend_images(ep, hp, gp, tp, dp, op, B, Hh, Wh, Hl, Wl, _stream()))
    else:
        _lib.check(_L().ff_fuse_blend(ep, hp, gp, tp, dp, op, Hh, Wh, Hl, Wl, _stream()))
    return out


@_instrument
def tile_accum(tile: T, wy: T, wx: T, acc: T, wsum: T, sy: int, sx: int):
    """acc [1,C,H,W] += tile [1,C,th,tw] * (wy x wx) at (sy, sx); wsum [1,1,H,W] += wy x wx."""
    _dev(tile, "tile_accum.tile", _F32)
    if tile.dim() != 4:
        raise _lib.FFError(f"tile_accum.tile: expected [1,C,th,tw], got {tuple(tile.shape)}")
    _, C, th, tw = tile.shape
    ap = _dense(acc, "tile_accum.acc", shape=(None, C, None, None))
    _, _, H, W = acc.shape
    tp = _dense(tile.contiguous(), "tile_accum.tile")
    wyp, wxp = _dense(wy, "tile_accum.wy", n=th), _dense(wx, "tile_accum.wx", n=tw)
    wsp = _dense(wsum, "tile_accum.wsum", n=H * W)
    _lib.check(_L().ff_tile_accum(tp, C, th, tw, wyp, wxp, ap, wsp, H, W, sy, sx, _stream()))


@_instrument
def tile_normalize(acc: T, wsum: T):
    ap = _dense(acc, "tile_normalize.acc", shape=(None, None, None, None))
    _, C, H, W = acc.shape
    wp = _dense(wsum, "tile_normalize.wsum", n=H * W)
    _lib.check(_L().ff_tile_normalize(ap, wp, C, H, W, _stream()))


D4_CODES = 16


def _d4_code(code) -> int:
    c = int(code)
    if not 0 <= c < D4_CODES:
        raise _lib.FFError(f"d4 code {c}: expected 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)")
    return c


def d4_check_codes(codes, H: int, W: int):
    """Host-side validation of augmentation codes (bit 0 hflip, bit 1 vflip, bits 2-3 k of rot90) for planes of H x W -> list of ints.
    Odd k swaps H and W: a batch must come out with one shape, so it needs square planes."""
    cl = [_d4_code(c) for c in codes]
    for c in cl:
        if (c >> 2) & 1 and H != W:
            raise _lib.FFError(f"d4 code {c} rotates by an odd quarter turn, which needs square planes, got {H}x{W}")
    return cl


def d4_nchw(x: T, codes, out: Optional[T] = None, codes_dev: Optional[T] = None) -> T:
    """The reference's paired augmentation (cached_dataset.py:240-268) of a planar batch [B,C,H,W]: sample b takes the symmetry
    codes[b] = hflip | vflip << 1 | k << 2, applied as flip(-1), flip(-2), rot90(k, (-2, -1)).  `codes` is a host sequence (checked
    here, before any launch); codes_dev, when given, is the same list already on the device (int32 [B]) so that the eight tensors
    of a micro-batch share one upload."""
    xp = _dense(x, "d4_nchw.x", shape=(None, None, None, None))
    B, C, H, W = x.shape
    cl = d4_check_codes(codes, H, W)
    if len(cl) != B:
        raise _lib.FFError(f"d4_nchw: {len(cl)} codes for a batch of {B}")
    if codes_dev is None:
        codes_dev = torch.tensor(cl, dtype=torch.int32).to(x.device)
    cp = _dense(codes_dev, "d4_nchw.codes_dev", _I32, n=B)
    out, op, _ = _out(out, "d4_nchw.out", tuple(x.shape), x.device, kind="dense")
    if op == xp:
        raise _lib.FFError("d4_nchw: out must be a distinct contiguous tensor of x's shape")
    _lib.check(_L().ff_d4_nchw(xp, op, B, C, H, W, cp, _stream()))
    return out


# The eight distinct symmetries of the square as d4 codes: k in {0, 1} times the four flip combinations (codes 8..15 repeat them:
# rot90(2) is both flips, rot90(3) is rot90(1) after both flips).
D4_ENSEMBLE = (0, 1, 2, 3, 4, 5, 6, 7)


def d4_inverse_code(code: int) -> int:
    """The d4 code whose transform undoes `code` (both read as flip(-1), flip(-2), rot90(k), in that order).  rot^k after exactly one
    flip is a reflection of the square, hence its own inverse; with none or both flips set (both = a half turn) the transform is a
    rotation, and its inverse keeps the flips and turns back: k' = (4 - k) % 4."""
    c = _d4_code(code)
    if (c & 1) != ((c >> 1) & 1):
        return c
    return (c & 3) | (((4 - (c >> 2)) % 4) << 2)


def d4_canonical_code(code: int) -> int:
    """The code in 0..7 (D4_ENSEMBLE) that names the same symmetry as `code`: a half turn is both flips, so k >= 2 toggles both flip
    bits and keeps k - 2."""
    c = _d4_code(code)
    return c if c < 8 else ((c & 3) ^ 3) | ((c >> 2) - 2) << 2


def d4_rect(x: T, code: int, out: Optional[T] = None, accum: bool = False, scale: float = 1.0) -> T:
    """ONE symmetry (`code` as in d4_nchw: flip(-1), flip(-2), rot90(k, (-2, -1))) of a planar [B,C,H,W] tensor of any H, W: the result
    is [B,C,H,W] for even k and [B,C,W,H] for odd k.  accum=False: out = t * scale; accum=True: out = (out + t) * scale, the add
    rounded before the multiply.  Everything is checked here, before the launch; `out` must not overlap x."""
    xp = _dense(x, "d4_rect.x", shape=(None, None, None, None))
    if x.numel() == 0:
        raise _lib.FFError("d4_rect: expected a non-empty contiguous [B,C,H,W] tensor")
    c = _d4_code(code)
    B, C, H, W = x.shape
    oshape = (B, C, W, H) if (c >> 2) & 1 else (B, C, H, W)
    if out is None and accum:
        raise _lib.FFError("d4_rect: accum=True needs the tensor to accumulate into (out)")
    if out is not None and isinstance(out, torch.Tensor) and out.device != x.device:
        raise _lib.FFError(f"d4_rect: out must be a contiguous {list(oshape)} tensor on x's device, got {list(out.shape)}")
    out, op, _ = _out(out, "d4_rect.out", oshape, x.device, kind="dense")
    nb = 4 * x.numel()
    if op < xp + nb and xp < op + nb:
        raise _lib.FFError("d4_rect: out overlaps x (the permutation is not in place)")
    _lib.check(_L().ff_d4_rect_nchw(xp, op, B, C, H, W, c, 1 if accum else 0, float(scale), _stream()))
    return out


def tile_cut_u8_d4(img_u8: T, code: int, y: int, x: int, th: int, tw: int, out: Optional[T] = None) -> T:
    """The th x tw tile at (y, x) of the TRANSFORMED image d4_rect(u8_to_f32_image(img_u8), code), which is never built: uint8 HWC
    [H,W,3] on the device -> fp32 [1,3,th,tw].  The transformed image is H x W for even k = code >> 2 and W x H for odd k; the tile
    must lie inside it.  Everything is checked here, before the launch."""
    ip = _dense(img_u8, "tile_cut_u8_d4.img_u8", _U8, shape=(None, None, 3))
    if img_u8.numel() == 0:
        raise _lib.FFError("tile_cut_u8_d4: expected a non-empty contiguous CUDA(HIP) uint8 [H,W,3] tensor")
    c, y, x, th, tw = _d4_code(code), int(y), int(x), int(th), int(tw)
    H, W, _ = img_u8.shape
    Ht, Wt = (W, H) if (c >> 2) & 1 else (H, W)
    if th < 1 or tw < 1 or y < 0 or x < 0 or y + th > Ht or x + tw > Wt:
        raise _lib.FFError(f"tile_cut_u8_d4: the {th}x{tw} tile at ({y},{x}) leaves the {Ht}x{Wt} transformed image (code {c} of a {H}x{W} image)")
    if out is None:
        out = torch.empty((1, 3, th, tw), device=img_u8.device, dtype=torch.float32)
    op = _dense(out, "tile_cut_u8_d4.out", n=3 * th * tw)
    if out.device != img_u8.device:
        raise _lib.FFError(f"tile_cut_u8_d4: out must be a contiguous float32 tensor of 3x{th}x{tw} elements on the image's device")
    _lib.check(_L().ff_tile_cut_u8_d4(ip, H, W, c, y, x, th, tw, op, _stream()))
    return out


def tile_fold_d4(acc: T, wsum: T, code: int, ens: Optional[T] = None, accum: bool = False, scale: float = 1.0) -> T:
    """One variant's un-normalised canvas folded into the ensemble accumulator in one pass: with v = acc / max(wsum, 1e-8)
    (tile_normalize's arithmetic) and t = d4_rect(v, code):  accum=False: ens = t * scale;  accum=True: ens = (ens + t) * scale, the
    add rounded before the multiply.  acc [1,3,Hc,Wc] and wsum [1,1,Hc,Wc] are only read; ens is [1,3,Hc,Wc] for even k = code >> 2 and
    [1,3,Wc,Hc] for odd k, and must overlap neither.  Everything is checked here, before the launch."""
    ap = _dense(acc, "tile_fold_d4.acc", shape=(1, 3, None, None))
    if acc.numel() == 0:
        raise _lib.FFError("tile_fold_d4: acc must be a non-empty contiguous [1,3,Hc,Wc] tensor")
    _, _, Hc, Wc = acc.shape
    wp = _dense(wsum, "tile_fold_d4.wsum", n=Hc * Wc)
    if tuple(wsum.shape[-2:]) != (Hc, Wc) or wsum.device != acc.device:
        raise _lib.FFError(f"tile_fold_d4: wsum must be a contiguous [1,1,{Hc},{Wc}] tensor on acc's device, got {list(wsum.shape)}")
    c = _d4_code(code)
    oshape = (1, 3, Wc, Hc) if (c >> 2) & 1 else (1, 3, Hc, Wc)
    if ens is None and accum:
        raise _lib.FFError("tile_fold_d4: accum=True needs the tensor to accumulate into (ens)")
    if ens is not None and isinstance(ens, torch.Tensor) and ens.device != acc.device:
        raise _lib.FFError(f"tile_fold_d4: ens must be a contiguous {list(oshape)} tensor on acc's device, got {list(ens.shape)}")
    ens, ep, _ = _out(ens, "tile_fold_d4.ens", oshape, acc.device, kind="dense")
    e1 = ep + 4 * ens.numel()
    for p_, t_, n_ in ((ap, acc, "acc"), (wp, wsum, "wsum")):
        if ep < p_ + 4 * t_.numel() and p_ < e1:
            raise _lib.FFError(f"tile_fold_d4: ens overlaps {n_} (the fold is not in place)")
    _lib.check(_L().ff_tile_fold_d4(ap, wp, Hc, Wc, c, ep, 1 if accum else 0, float(scale), _stream()))
    return ens


# ---- cached-expert data-set builder (cache.build_from_folders): patch pairs and the x1/4 degradation ---------------------------------
def crop_pairs_u8(lr_u8: T, hr_u8: T, positions, patch: int) -> Tuple[T, T]:
    """K aligned patch pairs out of one uploaded image pair, one launch: lr_u8 [h,w,3], hr_u8 [4h,4w,3] uint8 HWC on the device,
    positions = host sequence of LR (top, left) -> (lr [K,3,p,p], hr [K,3,4p,4p]) fp32 = u8 / 255, HR patch k at (4 top, 4 left).
    Everything, the positions included, is checked here before the launch."""
    lp = _dense(lr_u8, "crop_pairs_u8.lr_u8", _U8, shape=(None, None, 3))
    hp = _dense(hr_u8, "crop_pairs_u8.hr_u8", _U8, shape=(None, None, 3))
    for t, name in ((lr_u8, "lr_u8"), (hr_u8, "hr_u8")):
        if t.numel() == 0:
            raise _lib.FFError(f"crop_pairs_u8: {name} must be a non-empty contiguous CUDA(HIP) uint8 [H,W,3] tensor")
    if lr_u8.device != hr_u8.device:
        raise _lib.FFError("crop_pairs_u8: lr_u8 and hr_u8 are on different devices")
    h, w, _ = lr_u8.shape
    if tuple(hr_u8.shape) != (4 * h, 4 * w, 3):
        raise _lib.FFError(f"crop_pairs_u8: hr must be exactly 4x lr ({h}x{w}), got {hr_u8.shape[0]}x{hr_u8.shape[1]}")
    p = int(patch)
    if p < 1 or p > h or p > w:
        raise _lib.FFError(f"crop_pairs_u8: patch {p} does not fit the {h}x{w} LR image")
    pl = [(int(t_), int(l_)) for t_, l_ in positions]
    if not pl:
        raise _lib.FFError("crop_pairs_u8: no positions given")
    for t_, l_ in pl:
        if not (0 <= t_ <= h - p and 0 <= l_ <= w - p):
            raise _lib.FFError(f"crop_pairs_u8: position ({t_}, {l_}) puts a {p}x{p} patch outside the {h}x{w} LR image")
    K = len(pl)
    pos = torch.tensor(pl, dtype=torch.int32).to(lr_u8.device)
    lr, lrp, _ = _out(None, "crop_pairs_u8.lr", (K, 3, p, p), lr_u8.device, kind="dense")
    hr, hrp, _ = _out(None, "crop_pairs_u8.hr", (K, 3, 4 * p, 4 * p), lr_u8.device, kind="dense")
    _lib.check(_L().ff_crop_pairs_u8(lp, hp, h, w, _dense(pos, "crop_pairs_u8.pos", _I32, shape=(K, 2)), K, p, lrp, hrp, _stream()))
    _note(0.0, 17.0 * K * 3 * p * p * 5.0)
    return lr, hr


# ---- live-expert training (epoch.ImagePool / LiveEpoch): one micro-batch out of the resident image pool -----------------------------
def sample_pairs_u8(pool: T, desc_host, patch: int, desc_dev: Optional[T] = None, out: Optional[Tuple[T, T]] = None) -> Tuple[T, T]:
    """B augmented patch pairs out of one packed pool of uint8 HWC images, one launch (csrc/sample_batch.hip).  pool: 1-D uint8 device
    tensor; desc_host: host int64 [B][8] rows {lr_off, hr_off, h, w, top, left, code, 0} (byte offsets, LR image [h,w,3], HR partner
    [4h,4w,3], LR patch origin, d4 code) -> (lr [B,3,p,p], hr [B,3,4p,4p]) fp32 = u8 / 255, the bits of
    d4_nchw(crop_pairs_u8(...), codes).  Every row is checked here before the launch.  desc_dev: the same table already on the device
    (int64 [B,8]); out: (lr, hr) tensors to fill."""
    import numpy as np
    pp = _dense(pool, "sample_pairs_u8.pool", _U8, shape=(None,))
    if pool.numel() == 0:
        raise _lib.FFError("sample_pairs_u8: pool must be a non-empty contiguous 1-D CUDA(HIP) uint8 tensor")
    p = int(patch)
    d = np.ascontiguousarray(np.asarray(desc_host, dtype=np.int64))
    if d.ndim != 2 or d.shape[1] != 8 or d.shape[0] < 1 or p < 1:
        raise _lib.FFError(f"sample_pairs_u8: need B >= 1 rows of 8 fields and patch >= 1, got a table of shape {d.shape} and patch {p}")
    B, n = d.shape[0], pool.numel()
    for b in range(B):
        lo, ho, h, w, top, left, code, _ = (int(v) for v in d[b])
        if h < 1 or w < 1 or lo < 0 or ho < 0 or lo + 3 * h * w > n or ho + 48 * h * w > n:
            raise _lib.FFError(f"sample_pairs_u8: sample {b}: image {h}x{w} at byte offsets {lo} / {ho} leaves the pool of {n} bytes")
        if not (0 <= top <= h - p and 0 <= left <= w - p):
            raise _lib.FFError(f"sample_pairs_u8: sample {b}: position ({top}, {left}) puts a {p}x{p} patch outside the {h}x{w} LR image")
        if not 0 <= code < D4_CODES:
            raise _lib.FFError(f"sample_pairs_u8: sample {b}: d4 code {code}: expected 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)")
    if desc_dev is None:
        desc_dev = torch.from_numpy(d).to(pool.device)
    dp = _dense(desc_dev, "sample_pairs_u8.desc_dev", _I64, shape=(B, 8))
    if desc_dev.device != pool.device:
        raise _lib.FFError(f"sample_pairs_u8: desc_dev must be a contiguous int64 [{B}, 8] tensor on the pool's device")
    lr, hr = (None, None) if out is None else out
    for t in (lr, hr):
        if t is not None and isinstance(t, torch.Tensor) and t.device != pool.device:
            raise _lib.FFError(f"sample_pairs_u8: out must be contiguous {[B, 3, p, p]} and {[B, 3, 4 * p, 4 * p]} tensors on the pool's device")
    lr, lrp, _ = _out(lr, "sample_pairs_u8.out[0]", (B, 3, p, p), pool.device, kind="dense")
    hr, hrp, _ = _out(hr, "sample_pairs_u8.out[1]", (B, 3, 4 * p, 4 * p), pool.device, kind="dense")
    _lib.check(_L().ff_sample_pairs_u8(pp, dp, B, p, lrp, hrp, _stream()))
    _note(0.0, 17.0 * B * 3 * p * p * 5.0)
    return lr, hr


# ---- resident cached-expert training (epoch.ResidentCache / ResidentEpoch): one micro-batch out of the resident sample pool ----------
GATHER_MAX_FIELDS = 8


def gather_d4_fields(pool: T, n_samples: int, fields, desc_dev: T, out: T, desc_host=None):
    """One augmented micro-batch out of a field-major pool of cached samples, every field in one launch (csrc/gather_batch.hip).
    pool: 1-D fp32 device tensor; field f is a contiguous [n_samples, C, H, W] array that starts fields[f][0] floats into it.  fields:
    host int64 [F][5] rows {pool_off, out_off, C, H, W}, 1 <= F <= 8.  desc_dev: int32 [B, 2] device rows {sample index, d4 code}.  out:
    flat fp32 device tensor; field f of the batch is [B, C, H, W] at out[fields[f][1]:] = the bits of d4_nchw(field_f[index], codes).
    -> the F views of `out`.  Shapes, dtypes, extents and overlapping output fields are checked here before the launch; desc_host, the
    same table on the host, is checked too when given: indices in [0, n_samples), codes in 0..15, odd quarter turns only when every field
    is square.  (Without it the kernel's own guards hold: it clamps the index and drops the odd turn of a non-square field.)"""
    import numpy as np
    pp = _dense(pool, "gather_d4_fields.pool", shape=(None,))
    op = _dense(out, "gather_d4_fields.out", shape=(None,))
    for t, name in ((pool, "pool"), (out, "out")):
        if t.numel() < 1:
            raise _lib.FFError(f"gather_d4_fields: {name} must be a non-empty contiguous 1-D fp32 tensor")
    if out.device != pool.device:
        raise _lib.FFError("gather_d4_fields: out must be on the pool's device")
    n = int(n_samples)
    fl = np.ascontiguousarray(np.asarray(fields, dtype=np.int64))
    if fl.ndim != 2 or fl.shape[1] != 5 or not 1 <= fl.shape[0] <= GATHER_MAX_FIELDS or n < 1:
        raise _lib.FFError(f"gather_d4_fields: need 1..{GATHER_MAX_FIELDS} rows of 5 fields and n_samples >= 1, got a table of shape {fl.shape} and {n}")
    dp = _dense(desc_dev, "gather_d4_fields.desc_dev", _I32, shape=(None, 2))
    if desc_dev.shape[0] < 1 or desc_dev.device != pool.device:
        raise _lib.FFError("gather_d4_fields: desc_dev must be a contiguous int32 [B, 2] tensor (B >= 1) on the pool's device")
    B = int(desc_dev.shape[0])
    spans = []
    for f, (po, oo, C, H, W) in enumerate(fl.tolist()):
        if C < 1 or H < 1 or W < 1 or po < 0 or oo < 0:
            raise _lib.FFError(f"gather_d4_fields: field {f}: shape {C}x{H}x{W} at offsets {po} / {oo}")
        if po + n * C * H * W > pool.numel() or oo + B * C * H * W > out.numel():
            raise _lib.FFError(f"gather_d4_fields: field {f}: {n} samples of {C}x{H}x{W} at {po} leave the pool of {pool.numel()} floats, or "
                               f"{B} of them at {oo} the output of {out.numel()}")
        spans.append((oo, oo + B * C * H * W))
    spans.sort()
    if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
        raise _lib.FFError("gather_d4_fields: output fields overlap")
    if desc_host is not None:
        d = np.asarray(desc_host)
        if d.shape != (B, 2):
            raise _lib.FFError(f"gather_d4_fields: desc_host has shape {d.shape}, desc_dev [{B}, 2]")
        if ((d[:, 0] < 0) | (d[:, 0] >= n)).any():
            raise _lib.FFError(f"gather_d4_fields: sample index {int(d[:, 0].min())}..{int(d[:, 0].max())} outside the pool's 0..{n - 1}")
        for f in range(fl.shape[0]):                                  # odd quarter turns need square planes, in every field
            d4_check_codes(d[:, 1], int(fl[f, 3]), int(fl[f, 4]))
    _lib.check(_L().ff_gather_d4_fields(pp, n, fl.ctypes.data, int(fl.shape[0]), dp, B, op, _stream()))
    _note(0.0, 8.0 * B * float((fl[:, 2] * fl[:, 3] * fl[:, 4]).sum()))
    return [out[oo:oo + B * C * H * W].view(B, C, H, W) for _, oo, C, H, W in fl.tolist()]


def color_jitter_pairs(lr: T, hr: T, table_host, table_dev: Optional[T] = None) -> Tuple[T, T]:
    """The reference's paired colour jitter on a sampled micro-batch, IN PLACE, two launches (csrc/color_jitter.hip): lr [B,3,p,p] and
    hr [B,3,4p,4p] contiguous fp32 device tensors holding u8 / 255 (what sample_pairs_u8 writes); table_host: host fp32 [B][4] rows
    {apply, bf, cf, sf} -- apply 0 leaves the sample's two patches untouched, else brightness bf, contrast cf around each patch's own
    mean, saturation sf through the 8-bit HSV conversion (none when sf == 1).  Every row is checked here before the launch: apply in
    {0, 1}, factors finite and in (0, 2).  table_dev: the same table already on the device (fp32 [B,4]).  -> (lr, hr)."""
    import numpy as np
    lrp = _dense(lr, "color_jitter_pairs.lr", shape=(None, None, None, None))
    hrp = _dense(hr, "color_jitter_pairs.hr", shape=(None, None, None, None))
    B, p = int(lr.shape[0]), int(lr.shape[2])
    if B < 1 or p < 1 or tuple(lr.shape) != (B, 3, p, p) or tuple(hr.shape) != (B, 3, 4 * p, 4 * p) or hr.device != lr.device:
        raise _lib.FFError(f"color_jitter_pairs: need lr [B,3,p,p] and hr [B,3,4p,4p] on one device, got {list(lr.shape)} and {list(hr.shape)}")
    tb = np.ascontiguousarray(np.asarray(table_host, dtype=np.float32))
    if tb.shape != (B, 4):
        raise _lib.FFError(f"color_jitter_pairs: the table must be [{B}, 4] = {{apply, bf, cf, sf}}, got {tb.shape}")
    for b in range(B):
        ap, bf, cf, sf = (float(v) for v in tb[b])
        if ap not in (0.0, 1.0):
            raise _lib.FFError(f"color_jitter_pairs: sample {b}: apply is {ap}, expected 0 or 1")
        if not all(np.isfinite(v) and 0.0 < v < 2.0 for v in (bf, cf, sf)):
            raise _lib.FFError(f"color_jitter_pairs: sample {b}: factors ({bf}, {cf}, {sf}) must be finite and inside (0, 2)")
    if table_dev is None:
        table_dev = torch.from_numpy(tb).to(lr.device)
    tp = _dense(table_dev, "color_jitter_pairs.table_dev", shape=(B, 4))
    if table_dev.device != lr.device:
        raise _lib.FFError(f"color_jitter_pairs: table_dev must be a contiguous float32 [{B}, 4] tensor on lr's device")
    nbytes = int(_L().ff_color_jitter_workspace(B))
    work = torch.empty(nbytes // 8, device=lr.device, dtype=torch.int64)
    _lib.check(_L().ff_color_jitter_pairs(lrp, hrp, tp, B, p, _image(work, "color_jitter_pairs.work"), nbytes, _stream()))
    _note(0.0, 17.0 * float(tb[:, 0].sum()) * 3 * p * p * 4.0 * 3.0)  # applied samples: read for the sums, read and written by the pixel pass
    return lr, hr


AA_TAPS = 16


def _cubic_aa(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a
    return 0.0


def aa_tables(n_in: int, n_out: int):
    """Host tables of one axis of resize_aa (numpy): span int32 [n_out, 2] = (first input index, taps), wt float32 [n_out, 16].
    ATen's antialiased bicubic restated: s = n_in / n_out, centre s (i + 0.5), support 2 s, taps [int(c - 2s + 0.5), int(c + 2s + 0.5))
    clipped to the image, raw weight cubic_{a=-0.5}((j + first - c + 0.5) / s) in double, rounded to fp32, then divided by the
    fp32 sum of the row (summed in ascending j) -- border rows have fewer taps and renormalised weights."""
    import numpy as np
    if n_out < 1 or n_in < n_out:
        raise _lib.FFError(f"aa_tables: expected 1 <= n_out <= n_in, got {n_in} -> {n_out}")
    s = n_in / n_out
    span = np.zeros((n_out, 2), dtype=np.int32)
    wt = np.zeros((n_out, AA_TAPS), dtype=np.float32)
    for i in range(n_out):
        c = s * (i + 0.5)
        lo = max(int(c - 2.0 * s + 0.5), 0)
        hi = min(int(c + 2.0 * s + 0.5), n_in)
        if hi - lo > AA_TAPS:
            raise _lib.FFError(f"aa_tables: {n_in} -> {n_out} needs {hi - lo} taps, the kernel has {AA_TAPS}")
        raw = [np.float32(_cubic_aa((j + lo - c + 0.5) / s)) for j in range(hi - lo)]
        tot = np.float32(0.0)
        for v in raw:
            tot = np.float32(tot + v)
        span[i] = (lo, hi - lo)
        wt[i, :hi - lo] = [np.float32(v / tot) for v in raw]
    return span, wt


_AA_TABLES: Dict[tuple, Tuple[T, T]] = {}


def _aa_tables_dev(n_in: int, n_out: int, device) -> Tuple[T, T]:
    key = (n_in, n_out, str(device))
    ent = _AA_TABLES.get(key)
    if ent is None:
        if len(_AA_TABLES) >= 64:                       # a folder of images brings a handful of sizes; do not grow without bound
            _AA_TABLES.clear()
        span, wt = aa_tables(n_in, n_out)
        ent = _AA_TABLES[key] = (torch.from_numpy(span).to(device), torch.from_numpy(wt).to(device))
    return ent


def resize_aa(x: T, size: Tuple[int, int]) -> T:
    """Antialiased bicubic x1/4 of a planar image batch: x [B,3,H,W] -> [B,3,H/4,W/4] = F.interpolate(x, size, mode='bicubic',
    antialias=True, align_corners=False) -- the degradation the x4 track is defined on (ops.resize's bicubic is ATen's plain
    A = -0.75 kernel without antialiasing: an up-sampler).  `size` must be exactly (H/4, W/4); any other ratio raises."""
    xp = _dense(x, "resize_aa.x", shape=(None, 3, None, None))
    if x.numel() == 0:
        raise _lib.FFError("resize_aa: expected a non-empty contiguous [B,3,H,W] tensor")
    B, C, Hi, Wi = x.shape
    Ho, Wo = (int(v) for v in size)
    if Ho < 1 or Wo < 1 or Hi != 4 * Ho or Wi != 4 * Wo:
        raise _lib.FFError(f"resize_aa: only the x1/4 ratio is built: {Hi}x{Wi} -> {Ho}x{Wo} is refused")
    span_w, wt_w = _aa_tables_dev(Wi, Wo, x.device)
    span_h, wt_h = _aa_tables_dev(Hi, Ho, x.device)
    tabs = (_dense(span_w, "resize_aa.span_w", _I32, shape=(Wo, 2)), _dense(wt_w, "resize_aa.wt_w", shape=(Wo, AA_TAPS)),
            _dense(span_h, "resize_aa.span_h", _I32, shape=(Ho, 2)), _dense(wt_h, "resize_aa.wt_h", shape=(Ho, AA_TAPS)))
    out, op, _ = _out(None, "resize_aa.out", (B, C, Ho, Wo), x.device, kind="dense")
    _lib.check(_L().ff_resize_aa(xp, op, B * C, Hi, Wi, Ho, Wo, *tabs, _stream()))
    _note(0.0, 4.0 * B * C * (Hi * Wi + Ho * Wo))
    return out


def cv_cubic_tables(n_in: int, n_out: int):
    """Host tables of one axis of resize_cv_cubic (numpy): idx int32 [n_out, 4], wt float32 [n_out, 4].  OpenCV's INTER_CUBIC restated
    (resize.cpp, the table its resize builds per axis, and interpolateCubic): scale = double(n_in) / n_out,
    f = float32((d + 0.5) * scale - 0.5) with the product and the difference in double, s = floor(f), x = f - s in fp32; taps
    s - 1 .. s + 2, each clamped to [0, n_in - 1] (replicated border); weights in fp32 with A = -0.75f:
        c0 = ((A (x + 1) - 5 A)(x + 1) + 8 A)(x + 1) - 4 A,  c1 = ((A + 2) x - (A + 3)) x x + 1,
        c2 = ((A + 2)(1 - x) - (A + 3))(1 - x)(1 - x) + 1,   c3 = 1 - c0 - c1 - c2
    every operation rounded to fp32.  Any ratio, up or down: four taps, no antialiasing."""
    import numpy as np
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise _lib.FFError(f"cv_cubic_tables: sizes must be >= 1, got {n_in} -> {n_out}")
    F = np.float32
    scale = float(n_in) / float(n_out)
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f)
    x = (f - s).astype(F)
    A, one = F(-0.75), F(1)
    x1, u = x + one, one - x
    c0 = ((A * x1 - F(5) * A) * x1 + F(8) * A) * x1 - F(4) * A
    c1 = ((A + F(2)) * x - (A + F(3))) * x * x + one
    c2 = ((A + F(2)) * u - (A + F(3))) * u * u + one
    c3 = one - c0 - c1 - c2
    wt = np.stack([c0, c1, c2, c3], axis=1).astype(F)
    idx = np.clip(s.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1).astype(np.int32)
    return np.ascontiguousarray(idx), np.ascontiguousarray(wt)


_CVC_TABLES: Dict[tuple, Tuple[T, T]] = {}


def _cvc_tables_dev(n_in: int, n_out: int, device) -> Tuple[T, T]:
    key = (n_in, n_out, str(device))
    ent = _CVC_TABLES.get(key)
    if ent is None:
        if len(_CVC_TABLES) >= 64:                      # as _aa_tables_dev
            _CVC_TABLES.clear()
        idx, wt = cv_cubic_tables(n_in, n_out)
        ent = _CVC_TABLES[key] = (torch.from_numpy(idx).to(device), torch.from_numpy(wt).to(device))
    return ent


def resize_cv_cubic(x: T, Ho: int, Wo: int, out: Optional[T] = None, tables=None) -> T:
    """OpenCV's INTER_CUBIC restated, on the device (csrc/resample.hip): x [N,C,Hi,Wi] fp32 -> [N,C,Ho,Wo] = per plane
    cv2.resize(plane, (Wo, Ho), interpolation=cv2.INTER_CUBIC) as tests/golden/cv_cubic_ref.py restates it, bit for bit -- any ratio,
    four taps per axis, no antialiasing, replicated border, values not clamped.  Equal sizes give the input's bits.
    out: a contiguous [N,C,Ho,Wo] fp32 tensor to write (a view at any 4-byte offset).  tables: ((idx_w, wt_w), (idx_h, wt_h)) device
    tensors in cv_cubic_tables' shapes instead of the cached ones; anything else is refused before the launch.
    Parity with an OpenCV binary: unpinned (OpenCV absent)."""
    xp = _dense(x, "resize_cv_cubic.x", shape=(None, None, None, None))
    if x.numel() == 0:
        raise _lib.FFError(f"resize_cv_cubic: expected a non-empty contiguous [N,C,H,W] tensor, got {list(x.shape)}")
    N, C, Hi, Wi = x.shape
    Ho, Wo = int(Ho), int(Wo)
    if Ho < 1 or Wo < 1:
        raise _lib.FFError(f"resize_cv_cubic: the output size must be >= 1 x 1, got {Ho} x {Wo}")
    if tables is None:
        tw, th = _cvc_tables_dev(Wi, Wo, x.device), _cvc_tables_dev(Hi, Ho, x.device)
    else:
        try:
            (tw, th) = tables
            (iw, ww), (ih, wh) = tw, th
        except (TypeError, ValueError):
            raise _lib.FFError("resize_cv_cubic: tables must be ((idx_w, wt_w), (idx_h, wt_h))") from None
        for t in (iw, ww, ih, wh):
            if torch.is_tensor(t) and t.device != x.device:
                raise _lib.FFError("resize_cv_cubic: the tables must be contiguous int32 / float32 [n, 4] tensors on x's device")
    tabs = (_dense(tw[0], "resize_cv_cubic.tables.idx_w", _I32, shape=(Wo, 4)), _dense(tw[1], "resize_cv_cubic.tables.wt_w", shape=(Wo, 4)),
            _dense(th[0], "resize_cv_cubic.tables.idx_h", _I32, shape=(Ho, 4)), _dense(th[1], "resize_cv_cubic.tables.wt_h", shape=(Ho, 4)))
    if out is not None and isinstance(out, torch.Tensor) and out.device != x.device:
        raise _lib.FFError(f"resize_cv_cubic: out must be a contiguous [{N},{C},{Ho},{Wo}] tensor on x's device, got {list(out.shape)}")
    out, op, _ = _out(out, "resize_cv_cubic.out", (N, C, Ho, Wo), x.device, kind="dense")
    _lib.check(_L().ff_resize_cv_cubic(xp, op, N * C, Hi, Wi, Ho, Wo, *tabs, _stream()))
    _note(0.0, 4.0 * N * C * (Hi * Wi + Ho * Wo))
    return out
