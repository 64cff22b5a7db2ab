"""Torch-tensor front-end of the C ABI (include/ff_kernels.h).

PyTorch is plumbing here: it owns device memory and the stream.  Every function below only validates
shapes/strides and forwards raw pointers to libff_hip.so; there is no PyTorch compute fallback -- a
missing library or a CPU tensor raises.
Tensors are fp32, channel-last.  "rows view": any tensor whose last dim is contiguous and whose
leading dims collapse to a single row stride (e.g. a channel slice t[..., a:b] of an NHWC buffer).
"""
from __future__ import annotations

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
    import functools

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


def _split_weight(w: T, dynamic: bool, cin: int):
    """bf16 hi/lo planes [N][Kp] of a packed fp32 weight [N][taps*cin]; cached on the tensor object unless
    `dynamic`.  Per-tap padded (TAP) K layout when cin >= 32 and cin % 4 == 0, flat otherwise."""
    nterms = GEMM_MODES[_GEMM_MODE]
    cached = None if dynamic else PREPARED.peek(w, "split")
    if cached is not None and cached[4] >= nterms:
        return cached
    N, K = w.shape
    if cin >= 32 and cin % 4 == 0:
        Cp = (cin + 31) // 32 * 32
        Kp = (K // cin) * Cp
    else:
        Cp, Kp = 0, (K + 31) // 32 * 32
    hi = torch.empty((N, Kp), device=w.device, dtype=torch.bfloat16)
    lo = torch.empty((N, Kp), device=w.device, dtype=torch.bfloat16) if nterms == 3 else None
    _lib.check(_L().ff_split_bf16(w.data_ptr(), N, K, Kp, cin, Cp, hi.data_ptr(), lo.data_ptr() if lo is not None else None,
                                  _stream()))
    ent = (hi, lo, Kp, Cp, nterms)
    if not dynamic:
        PREPARED.put(w, "split", ent)
    return ent


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk(t: T, name: str):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (t.dtype != torch.float32 and not (t.dtype == torch.bfloat16 and name.endswith("|bf16ok"))):
        raise _lib.FFError(f"{name.split('|')[0]}: expected a CUDA(HIP) float32 tensor")


def _ptr(t: Optional[T]) -> Optional[int]:
    if t is None:
        return None
    _chk(t, "arg")
    return t.data_ptr()


def rows_view(t: T, name: str = "tensor") -> Tuple[int, int, int, int]:
    """-> (ptr, ld, rows, C) for a tensor whose leading dims collapse to rows of stride ld."""
    _chk(t, name)
    if t.dim() == 1:
        return t.data_ptr(), t.shape[0], 1, t.shape[0]
    if t.stride(-1) != 1 and t.shape[-1] != 1:
        raise _lib.FFError(f"{name}: last dim must be contiguous")
    ld = t.stride(-2)
    rows = 1
    expect = ld
    for d in range(t.dim() - 2, -1, -1):
        if t.shape[d] != 1 and t.stride(d) != expect:
            raise _lib.FFError(f"{name}: leading dims do not collapse to a constant row stride {tuple(t.shape)} {t.stride()}")
        expect = expect * t.shape[d]
        rows *= t.shape[d]
    return t.data_ptr(), ld, rows, t.shape[-1]


def _nhwc(t: T, name: str):
    """-> (ptr, ld, B, H, W, C) for a 4-D NHWC rows view."""
    if t.dim() != 4:
        raise _lib.FFError(f"{name}: expected [B,H,W,C]")
    p, ld, rows, c = rows_view(t, name)
    return p, ld, t.shape[0], t.shape[1], t.shape[2], c


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
    per_image = bool(per_image or want_pool) and x.dim() == 4 and x.shape[0] > 1
    in_bf16 = x.dtype == torch.bfloat16
    xp, ldi, B, H, W, Cin = _nhwc(x, "conv2d.x|bf16ok" if in_bf16 else "conv2d.x")
    KH, KW = ksize
    Cout = w.shape[0]
    if w.dim() != 2 or w.shape[1] != KH * KW * Cin or not w.is_contiguous():
        raise _lib.FFError(f"conv2d: packed weight must be [Cout, {KH * KW * Cin}], got {tuple(w.shape)}")
    Ho = (H + 2 * pad[0] - KH) // stride[0] + 1
    Wo = (W + 2 * pad[1] - KW) // stride[1] + 1
    oshape = (B, Ho * 2, Wo * 2, Cout // 4) if shuffle == 2 else (B, Ho, Wo, Cout)
    if out is None:
        out = empty_rows_bf16(oshape, x.device) if out_bf16 else empty_rows(oshape, x.device)
    elif tuple(out.shape) != oshape:
        raise _lib.FFError(f"conv2d: out shape {tuple(out.shape)} != {oshape}")
    out_bf16 = out.dtype == torch.bfloat16
    op, ldo, *_ = _nhwc(out, "conv2d.out|bf16ok" if out_bf16 else "conv2d.out")
    halo_ok = (_HALO and _GEMM_MODE in ("bf16x3", "bf16") and (KH, KW) == (3, 3) and tuple(stride) == (1, 1) and tuple(pad) == (1, 1)
               and not dynamic_w and Cin >= 32 and Cin % 4 == 0 and ldi % 4 == 0 and xp % 16 == 0
               and (Cout <= 64 or Cin >= 128 or 128 < Cout <= 192)   # measured (profiles/r01_conv3x3_halo_vs_igemm.txt); 64 -> 256 ties
               and H * W >= 1024 and xp != op and B * H * W * ldi < 2 ** 31)
    # (the last term is the one condition that counts the whole launch: the kernel's 32-bit offsets.  A caller that batches independent
    # images keeps its batches below it -- HatHIP.forward sizes its chunks so -- and every other term is one image's.)
    if (in_bf16 or out_bf16) and not (halo_ok and _GEMM_MODE == "bf16" and shuffle == 0 and res is None):
        raise _lib.FFError("conv2d: bf16 input / output rows exist for the LDS-resident 3x3 kernel in plain-bf16 mode only")
    rp, ldr = None, 0
    if res is not None:
        if tuple(res.shape) != oshape:
            raise _lib.FFError(f"conv2d: res shape {tuple(res.shape)} != {oshape}")
        rp, ldr, *_ = _nhwc(res, "conv2d.res")
    if (_GEMM_MODE != "f32" and (KH, KW) == (3, 3) and tuple(stride) == (1, 1) and tuple(pad) == (1, 1) and Cout <= 16
            and Cin * (1 if Cout == 1 else (4 if Cout <= 4 else 16)) <= 128 and shuffle == 0 and mul is None and not dynamic_w and H * W >= 4096 and xp != op):
        # small-channel tail convolutions: exact fp32 on the VALU from an LDS halo tile (csrc/conv3x3_small.hip).  Measured on
        # MI355X at 1024 x 1024: 16->3 205 -> <70 us, 8->1 160 -> <70, 16->1 204 -> <70, 32->3 166 -> 95, 6->16 173 -> 126; but
        # 64->3 202 -> 370 and 32->16 187 -> 199 (VALU-bound: Cin * CT FMAs per pixel and tap), hence the Cin * CT <= 128 rule
        from . import prep as _prep
        ws = PREPARED.get(w, "small", lambda: _prep.pack_conv3x3_small(w, Cin))
        _lib.check(_L().ff_conv3x3_small(xp, ldi, ws.data_ptr(), ws.shape[2], _ptr(bias), rp, ldr, op, ldo, B, H, W, Cin, Cout, ACT[act],
                                         float(alpha), _stream()))
    elif _GEMM_MODE == "f32":
        _lib.check(_L().ff_conv2d(xp, w.data_ptr(), _ptr(bias), _ptr(mul), rp, op, B, H, W, Cin, ldi, Ho, Wo, Cout, ldo, ldr,
                                  KH, KW, stride[0], stride[1], pad[0], pad[1], ACT[act], float(alpha), shuffle, tile_hint,
                                  _stream()))
    elif halo_ok:
        from . import prep as _prep

        nt_ = _nterms()

        def _mk_halo():
            bn = _prep.halo_bn(Cout)
            return (_prep.pack_conv3x3_halo(w, Cin, bn, nt_), bn)
        img = PREPARED.get(w, "halo" if nt_ == 3 else "halo1", _mk_halo)
        part = None
        halo_fn, rows_fn = ((_L().ff_conv3x3_halo_images, _L().ff_conv3x3_halo_images_pool_rows) if per_image else
                            (_L().ff_conv3x3_halo, _L().ff_conv3x3_halo_pool_rows))
        if want_pool and (B == 1 or per_image) and shuffle == 0 and Cout <= img[1]:
            prow = int(rows_fn(B, H, W, Cout, img[1], nt_))
            part = torch.empty((prow, img[1]), device=x.device, dtype=torch.float32)
        _lib.check(halo_fn(xp, ldi, img[0].data_ptr(), img[1], _ptr(bias), _ptr(mul), rp, ldr, op, ldo, B, H, W,
                           Cin, Cout, ACT[act], float(alpha), shuffle, _ptr(part), _nterms(),
                           (1 if in_bf16 else 0) | (2 if out_bf16 else 0), _stream()))
        if part is not None:
            pp = PoolPartials(part, Cout, 1.0 / float(H * W), images=B)
            _note(2.0 * B * Ho * Wo * Cout * KH * KW * Cin, 4.0 * (_numel(x, w, out, res)))
            return out, (pp if want_pool == "partials" else pp.mean())
    else:
        aligned = (ldi % 4 == 0) and (xp % 16 == 0)
        hi, lo, Kp, Cp, _ = _split_weight(w, dynamic_w, Cin if aligned else 0)
        if per_image and tile_hint <= 0:                    # the tile configuration one image's launch picks for itself
            tile_hint = int(_L().ff_conv2d_bf16s_tile(Ho * Wo, Cout, KH * KW * Cin, 1 if aligned and Cin % 4 == 0 else 0))
        _lib.check(_L().ff_conv2d_bf16s(xp, hi.data_ptr(), lo.data_ptr() if lo is not None else None, Kp, Cp, _ptr(bias), _ptr(mul),
                                        rp, op, B, H, W, Cin, ldi, Ho, Wo, Cout, ldo, ldr, KH, KW, stride[0], stride[1],
                                        pad[0], pad[1], ACT[act], float(alpha), shuffle, GEMM_MODES[_GEMM_MODE], tile_hint,
                                        None, _stream()))
    _note(2.0 * B * Ho * Wo * Cout * KH * KW * Cin, 4.0 * (_numel(x, w, out, res)))
    if want_pool:
        return out, pool_mean(out)
    return out


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
    xp, ldi, rows, K = rows_view(x, "linear.x")
    N = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K or not w.is_contiguous():
        raise _lib.FFError(f"linear: weight must be [N, {K}], got {tuple(w.shape)}")
    if (kmul is not None or gate_pairs) and _GEMM_MODE == "f32":
        raise _lib.FFError("linear: kmul / gate_pairs exist in the split-bf16 kernels only")
    No = N // 2 if gate_pairs else N
    oshape = tuple(x.shape[:-1]) + (No,)
    if out is None:
        out = empty_rows(oshape, x.device)
    op, ldo, orows, oc = rows_view(out, "linear.out")
    if orows != rows or oc != No:
        raise _lib.FFError("linear: out shape mismatch")
    rp, ldr = None, 0
    if res is not None:
        rp, ldr, rrows, rc = rows_view(res, "linear.res")
        if rrows != rows or rc != N:
            raise _lib.FFError("linear: res shape mismatch")
    if rows_per_image and rows % rows_per_image:
        raise _lib.FFError(f"linear: {rows} rows are not whole images of rows_per_image = {rows_per_image} rows")
    if _GEMM_MODE == "f32":
        _lib.check(_L().ff_conv2d(xp, w.data_ptr(), _ptr(bias), _ptr(mul), rp, op, 1, 1, rows, K, ldi, 1, rows, N, ldo, ldr,
                                  1, 1, 1, 1, 0, 0, ACT[act], float(alpha), 0, 0, _stream()))
    else:
        aligned = (ldi % 4 == 0) and (xp % 16 == 0)
        images = _kmul_images(kmul, K, rows)                 # (refusals first: nothing is launched, no weight is split, before them)
        if images > 1 and (act is not None or alpha != 1.0 or gate_pairs or not aligned or K % 4 or N % 4):
            raise _lib.FFError("linear: kmul [B, K] comes with the (bias, * mul, + res) epilogue on 16-byte aligned rows only")
        hi, lo, Kp, Cp, _ = _split_weight(w, dynamic_w, K if aligned else 0)
        if images > 1:
            _lib.check(_L().ff_conv2d_bf16s_kmul_images(xp, ldi, hi.data_ptr(), lo.data_ptr() if lo is not None else None, Kp, Cp,
                                                        kmul.data_ptr(), images, rows // images, _ptr(bias), _ptr(mul), rp, ldr, op, ldo,
                                                        rows, K, N, GEMM_MODES[_GEMM_MODE], 0, _stream()))
        else:
            hint = 0                                         # several images: the tile configuration one image's launch picks for itself
            if rows_per_image and rows_per_image != rows:
                hint = int(_L().ff_conv2d_bf16s_tile(rows_per_image, N, K, 1 if aligned and K % 4 == 0 else 0))
            _lib.check(_L().ff_conv2d_bf16s(xp, hi.data_ptr(), lo.data_ptr() if lo is not None else None, Kp, Cp, _ptr(bias), _ptr(mul),
                                            rp, op, 1, 1, rows, K, ldi, 1, rows, N, ldo, ldr, 1, 1, 1, 1, 0, 0, ACT[act],
                                            float(alpha), 1 if gate_pairs else 0, GEMM_MODES[_GEMM_MODE], hint, _ptr(kmul), _stream()))
    _note(2.0 * rows * N * K, 4.0 * (rows * K + N * K + rows * No * (2 if res is not None else 1)))
    return out


def _linear_wimages(x: T, w: T, bias, *, act, res, mul, alpha, out, dynamic_w, kmul, gate_pairs, out_bf16, tile_hint, rows_gemm) -> T:
    """linear with one weight matrix per image, w [B, N, K].  Every refusal comes before the weight split and the launch."""
    _chk(w, "linear.w")
    B, N, K = w.shape
    if _GEMM_MODE == "f32" or not dynamic_w or not w.is_contiguous():
        raise _lib.FFError("linear: per-image weights [B, N, K] are contiguous dynamic weights (dynamic_w=True) of the split-bf16 modes")
    if (x.dtype != torch.float32 or rows_gemm or kmul is not None or gate_pairs or out_bf16 or tile_hint or act is not None
            or alpha != 1.0):
        raise _lib.FFError("linear: per-image weights come with fp32 rows and the (bias, * mul, + res) epilogue only")
    xp, ldi, rows, xk = rows_view(x, "linear.x")
    if xk != K or rows % B or (rows // B) % 256:
        raise _lib.FFError(f"linear: per-image weights {tuple(w.shape)} need [rows, {K}] input with B = {B} equal groups of a multiple of "
                           f"256 rows, got {rows} rows of {xk}")
    if ldi % 4 or xp % 16 or K % 4 or N % 4:
        raise _lib.FFError("linear: per-image weights need 16-byte aligned rows, K % 4 == 0 and N % 4 == 0")
    oshape = tuple(x.shape[:-1]) + (N,)
    if out is None:
        out = empty_rows(oshape, x.device)
    op, ldo, orows, oc = rows_view(out, "linear.out")
    if orows != rows or oc != N or ldo % 4 or op % 16:
        raise _lib.FFError("linear: out shape mismatch (per-image weights: 16-byte aligned rows)")
    rp, ldr = None, 0
    if res is not None:
        rp, ldr, rrows, rc = rows_view(res, "linear.res")
        if rrows != rows or rc != N or ldr % 4 or rp % 16:
            raise _lib.FFError("linear: res shape mismatch (per-image weights: 16-byte aligned rows)")
    hi, lo, Kp, Cp, _ = _split_weight(w.reshape(B * N, K), True, K)        # rows are split independently: image b's planes at [b * N, (b + 1) * N)
    _lib.check(_L().ff_conv2d_bf16s_wimages(xp, ldi, hi.data_ptr(), lo.data_ptr() if lo is not None else None, Kp, Cp, B, rows // B,
                                            _ptr(bias), _ptr(mul), rp, ldr, op, ldo, rows, K, N, GEMM_MODES[_GEMM_MODE], 0, _stream()))
    _note(2.0 * rows * N * K, 4.0 * (rows * K + B * N * K + rows * N * (2 if res is not None else 1)))
    return out


def _kmul_images(kmul: Optional[T], K: int, rows: int) -> int:
    """linear's kmul: [K] (or [1, K]) -> 1; a contiguous [B, K] matrix with B > 1 dividing the row count -> B; anything else raises."""
    if kmul is None:
        return 1
    _chk(kmul, "linear.kmul")
    if not kmul.is_contiguous() or kmul.numel() % K or (kmul.numel() != K and (kmul.dim() != 2 or kmul.shape[1] != K)):
        raise _lib.FFError(f"linear: kmul must be a contiguous [{K}] vector or [B, {K}] matrix, got {tuple(kmul.shape)}")
    images = kmul.numel() // K
    if images < 1 or rows % images:
        raise _lib.FFError(f"linear: kmul {tuple(kmul.shape)} needs a row count that B = {images} divides, got {rows} rows")
    return images


def rows_gemm_ok(K: int) -> bool:
    """Shapes ff_gemm_rows_bf16 takes: whole 64-wide K chunks, so that the weight plane of _split_weight is unpadded."""
    return K % 64 == 0


def _linear_rows_bf16(x: T, w: T, bias, *, act, res, mul, alpha, out, dynamic_w, kmul, gate_pairs, out_bf16, tile_hint) -> T:
    xp, lda, rows, K = rows_view(x, "linear.x|bf16ok")
    a32 = x.dtype == torch.float32
    N = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K or not w.is_contiguous():
        raise _lib.FFError(f"linear: weight must be [N, {K}], got {tuple(w.shape)}")
    if _GEMM_MODE != "bf16" or not rows_gemm_ok(K):
        raise _lib.FFError("linear: the bf16-rows GEMM exists in plain-bf16 mode for K % 64 == 0 only")
    if kmul is not None and not a32:
        raise _lib.FFError("linear: kmul scales fp32 input rows only")
    images = _kmul_images(kmul, K, rows)
    if act is not None or alpha != 1.0 or (a32 and gate_pairs) or (gate_pairs and (res is not None or mul is not None)) or out_bf16 != gate_pairs:
        raise _lib.FFError("linear: the bf16-rows GEMM has three epilogues: bias (* mul + res) -> fp32 rows, or the SimpleGate pair "
                           "product -> bf16 rows")
    No = N // 2 if gate_pairs else N
    oshape = tuple(x.shape[:-1]) + (No,)
    if out is None:
        out = empty_rows_bf16(oshape, x.device) if out_bf16 else empty_rows(oshape, x.device)
    elif (out.dtype == torch.bfloat16) != out_bf16:
        raise _lib.FFError("linear: out dtype does not match out_bf16")
    op, ldo, orows, oc = rows_view(out, "linear.out|bf16ok" if out_bf16 else "linear.out")
    if orows != rows or oc != No:
        raise _lib.FFError("linear: out shape mismatch")
    rp, ldr = None, 0
    if res is not None:
        rp, ldr, rrows, rc = rows_view(res, "linear.res")
        if rrows != rows or rc != N:
            raise _lib.FFError("linear: res shape mismatch")
    hi, _, Kp, _, _ = _split_weight(w, dynamic_w, K)
    if images > 1:
        _lib.check(_L().ff_gemm_rows_bf16_kmul_images(xp, lda, hi.data_ptr(), Kp, kmul.data_ptr(), images, rows // images, _ptr(bias), _ptr(mul),
                                                      rp, ldr, op, ldo, rows, N, K, int(tile_hint), _stream()))
    else:
        _lib.check(_L().ff_gemm_rows_bf16(xp, 1 if a32 else 0, lda, hi.data_ptr(), Kp, _ptr(kmul), _ptr(bias), _ptr(mul), rp, ldr, op, ldo, rows,
                                          N, K, 1 if gate_pairs else 0, int(tile_hint), _stream()))
    _note(2.0 * rows * N * K, (4.0 if a32 else 2.0) * rows * K + 2.0 * N * K + (2.0 if out_bf16 else 4.0) * rows * No + (4.0 * rows * No if res is not None else 0.0))
    return out


def window_attn(qkv: T, out: T, biasT: T, *, q_off: int, k_off: int, v_off: int, o_off: int, H: int, W: int, Hp: int,
                Wp: int, win: Tuple[int, int], kwin: Tuple[int, int], shift: Tuple[int, int], use_mask: bool, heads: int,
                d: int, scale: float, rel_table: Optional[T] = None) -> T:
    qp, ldq, B, h_, w_, _ = _nhwc(qkv, "window_attn.qkv")
    op, ldo, *_ = _nhwc(out, "window_attn.out")
    if (h_, w_) != (H, W) or tuple(out.shape[:3]) != (B, H, W):
        raise _lib.FFError("window_attn: qkv/out spatial dims mismatch")
    nk = kwin[0] * kwin[1]
    if tuple(biasT.shape) != (heads, nk, 256) or not biasT.is_contiguous():
        raise _lib.FFError(f"window_attn: biasT must be [{heads},{nk},256]")
    if q_off + heads * d > qkv.shape[-1] or k_off + heads * d > qkv.shape[-1] or v_off + heads * d > qkv.shape[-1] \
            or o_off + heads * d > out.shape[-1]:
        raise _lib.FFError("window_attn: channel offsets out of range")
    if _GEMM_MODE == "f32":
        _lib.check(_L().ff_window_attn(qp, ldq, q_off, k_off, v_off, op, ldo, o_off, biasT.data_ptr(), B, H, W, Hp, Wp, win[0],
                                       win[1], kwin[0], kwin[1], shift[0], shift[1], int(use_mask), heads, d, float(scale),
                                       _stream()))
    else:
        relp = None
        if rel_table is not None and tuple(kwin) != tuple(win):
            # overlapping keys: the rotated table of prep.pack_rel_overlap, gathered in the kernel through a per-key offset table
            n = (win[0] + kwin[0] - 1) * (win[1] + kwin[1] - 1)
            if tuple(rel_table.shape) != (heads, n) or not rel_table.is_contiguous() or kwin[1] % 8 or tuple(shift) != (0, 0):
                raise _lib.FFError(f"window_attn: overlapping-window rel_table must be [heads, {n}] (prep.pack_rel_overlap), kw % 8 == 0, no shift")
            relp = rel_table.data_ptr()
        elif rel_table is not None and tuple(kwin) == tuple(win) and win[1] & (win[1] - 1) == 0 and win[1] >= 8:
            if tuple(rel_table.shape) != (heads, (2 * win[0] - 1) * (2 * win[1] - 1)) or not rel_table.is_contiguous():
                raise _lib.FFError("window_attn: rel_table must be [heads, (2wh-1)*(2ww-1)]")
            relp = rel_table.data_ptr()
        from . import prep as _prep
        bq = PREPARED.get(biasT, "quad", lambda: _prep.quad_bias(biasT))          # load-time relayout, once per table
        _lib.check(_L().ff_window_attn_bf16s(qp, ldq, q_off, k_off, v_off, op, ldo, o_off, bq.data_ptr(), B, H, W, Hp, Wp,
                                             win[0], win[1], kwin[0], kwin[1], shift[0], shift[1], int(use_mask), heads, d,
                                             float(scale), 1 if _GEMM_MODE == "bf16" else 3, relp, _stream()))
    nwin = B * (Hp // win[0]) * (Wp // win[1])
    _note(4.0 * nwin * heads * 256 * nk * d, 4.0 * (4.0 * B * H * W * heads * d + heads * nk * 256))
    return out


def ocab_attn(qkv: T, out: T, rel_rotated: T, *, q_off: int, k_off: int, v_off: int, o_off: int = 0, H: int, W: int, heads: int, d: int,
              ws: int, ows: int, scale: float) -> T:
    """HAT OCAB attention stage in one persistent-workgroup launch (plain bf16; csrc/ocab_attn.hip): 16x16 query windows against
    24x24 zero-padded key windows, bias from the rotated compact table of prep.pack_rel_overlap [heads, 39*39]."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("ocab_attn exists for the plain-bf16 contraction mode only")
    qp, ldq, B, h_, w_, _ = _nhwc(qkv, "ocab_attn.qkv")
    out_bf16 = out.dtype == torch.bfloat16
    op, ldo, *_ = _nhwc(out, "ocab_attn.out|bf16ok" if out_bf16 else "ocab_attn.out")
    if (h_, w_) != (H, W) or tuple(out.shape[:3]) != (B, H, W) or tuple(rel_rotated.shape) != (heads, (ws + ows - 1) ** 2) or not rel_rotated.is_contiguous():
        raise _lib.FFError("ocab_attn: shape mismatch")
    _lib.check(_L().ff_ocab_attn(qp, ldq, q_off, k_off, v_off, op, ldo, o_off, rel_rotated.data_ptr(), B, H, W, heads, d, ws, ows,
                                 float(scale), int(out_bf16), _stream()))
    nwin = B * (H // ws) * (W // ws)
    _note(4.0 * nwin * heads * ws * ws * ows * ows * d, 4.0 * B * H * W * heads * d * 4)
    return out


def ocab_attn_rows16(qkv16: T, out: T, rel_rotated: T, *, q_off: int, k_off: int, v_off: int, o_off: int = 0, H: int, W: int, heads: int,
                     d: int, ws: int, ows: int) -> T:
    """ocab_attn on the head-padded bf16 rows of token_linear_rows16 (csrc/ocab_attn.hip, ROWS16): head h of q / k / v at
    q_off / k_off / v_off + 32 h, q already scaled."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("ocab_attn_rows16 exists for the plain-bf16 contraction mode only")
    if qkv16.dtype != torch.bfloat16:
        raise _lib.FFError("ocab_attn_rows16: qkv must be bf16 rows")
    qp, ldq, B, h_, w_, _ = _nhwc(qkv16, "ocab_attn_rows16.qkv|bf16ok")
    out_bf16 = out.dtype == torch.bfloat16
    op, ldo, *_ = _nhwc(out, "ocab_attn_rows16.out|bf16ok" if out_bf16 else "ocab_attn_rows16.out")
    if (h_, w_) != (H, W) or tuple(out.shape[:3]) != (B, H, W) or tuple(rel_rotated.shape) != (heads, (ws + ows - 1) ** 2) or not rel_rotated.is_contiguous():
        raise _lib.FFError("ocab_attn_rows16: shape mismatch")
    if max(q_off, k_off, v_off) + heads * 32 > qkv16.shape[-1]:
        raise _lib.FFError("ocab_attn_rows16: channel offsets out of range")
    _lib.check(_L().ff_ocab_attn_rows16(qp, ldq, q_off, k_off, v_off, op, ldo, o_off, rel_rotated.data_ptr(), B, H, W, heads, d, ws, ows,
                                        int(out_bf16), _stream()))
    nwin = B * (H // ws) * (W // ws)
    _note(4.0 * nwin * heads * ws * ws * ows * ows * d, B * H * W * heads * (2.0 * 3 * 32 + (2.0 if out_bf16 else 4.0) * d))
    return out


def win_attn_fused(x: T, out: T, pk: dict, rel_padded: T, *, gamma: Optional[T], beta: Optional[T], eps: float = 1e-5,
                   H: int, W: int, Hp: int, Wp: int, win: Tuple[int, int], shift: Tuple[int, int], use_mask: bool,
                   head0: int = 0, nheads: Optional[int] = None, o_off: int = 0, zero_pad: bool = False,
                   want_xn: bool = False, v_out: Optional[T] = None, v_off: int = 0):
    """LayerNorm + qkv projection + window attention of `nheads` heads in one launch (csrc/win_attn_fused.hip); pk from
    prep.pack_win_attn, rel_padded from prep.pack_win_rel.  x [B,H,W,K] rows view; out [B,H,W,>= o_off + heads*d].
    want_xn: also return the normalised rows; v_out: receives v of the processed heads at channel v_off + g*d."""
    xp, ldx, B, h_, w_, K = _nhwc(x, "win_attn_fused.x")
    out_bf16 = out.dtype == torch.bfloat16
    op, ldo, *_ = _nhwc(out, "win_attn_fused.out|bf16ok" if out_bf16 else "win_attn_fused.out")
    xn_bf16 = want_xn == "bf16"
    if (out_bf16 or xn_bf16) and _GEMM_MODE != "bf16":
        raise _lib.FFError("win_attn_fused: bf16 outputs exist for the plain-bf16 contraction mode only")
    if (h_, w_) != (H, W) or tuple(out.shape[:3]) != (B, H, W) or K != pk["K"]:
        raise _lib.FFError("win_attn_fused: x/out dims mismatch")
    nheads = pk["heads"] - head0 if nheads is None else nheads
    if tuple(rel_padded.shape[:2]) != (pk["heads"], 2 * win[0] - 1) or not rel_padded.is_contiguous():
        raise _lib.FFError("win_attn_fused: rel_padded must be [heads][2wh-1][stride]")
    if _GEMM_MODE not in ("bf16x3", "bf16"):
        raise _lib.FFError("win_attn_fused exists for the bf16 contraction modes only")
    xn, xnp, ldxn = None, None, 0
    if want_xn:
        xn = empty_rows_bf16(tuple(x.shape), x.device) if xn_bf16 else empty_like_rows(x)
        xnp, ldxn, _, _ = rows_view(xn, "win_attn_fused.xn|bf16ok" if xn_bf16 else "win_attn_fused.xn")
    vp, ldv = None, 0
    if v_out is not None:
        vp, ldv, vb, vh, vw, _ = _nhwc(v_out, "win_attn_fused.v_out")
        if (vb, vh, vw) != (B, H, W):
            raise _lib.FFError("win_attn_fused: v_out dims mismatch")
    _lib.check(_L().ff_win_attn_fused(xp, ldx, op, ldo, o_off, _ptr(gamma), _ptr(beta), float(eps), pk["w"].data_ptr(),
                                      pk["b"].data_ptr(), rel_padded.data_ptr(), rel_padded.shape[1], rel_padded.shape[2], B, H, W,
                                      Hp, Wp, win[0], win[1], shift[0], shift[1], int(use_mask), head0, nheads, pk["d"], K,
                                      int(zero_pad), xnp, ldxn, vp, ldv, v_off, 1 if _GEMM_MODE == "bf16" else 3, int(out_bf16), int(xn_bf16),
                                      _stream()))
    nwin = B * (Hp // win[0]) * (Wp // win[1])
    _note(2.0 * nwin * 256 * K * 3 * nheads * pk["d"] + 4.0 * nwin * nheads * 256 * 256 * pk["d"],
          4.0 * B * H * W * (K * (1 + (0 if not want_xn else (0.5 if xn_bf16 else 1.0))) + nheads * pk["d"] * ((0.5 if out_bf16 else 1.0) + (1 if v_out is not None else 0))))
    return (out, xn) if want_xn else out


def token_mlp(x: T, gamma: T, beta: T, pk: dict, eps: float = 1e-5) -> T:
    """x + fc2(GELU(fc1(LayerNorm(x)))) in one launch (bf16x3 only); pk from prep.pack_token_mlp."""
    xp, ldx, rows, K = rows_view(x, "token_mlp.x")
    if K != pk["K"] or pk["N"] != K:
        raise _lib.FFError("token_mlp: shape mismatch")
    out = empty_like_rows(x)
    op_, ldo_, _, _ = rows_view(out, "token_mlp.out")
    _lib.check(_L().ff_token_mlp(xp, ldx, op_, ldo_, rows, K, pk["ht"], pk["N"], gamma.data_ptr(), beta.data_ptr(),
                                 float(eps), pk["w"].data_ptr(), pk["b1"].data_ptr(), pk["b2"].data_ptr(), _nterms(), _stream()))
    _note(4.0 * rows * K * pk["ht"] * 32, 8.0 * rows * K)
    return out


def token_projmlp(att: T, x: T, pk: dict, gamma: T, beta: T, *, c2: Optional[T] = None, c2_scale: Optional[T] = None,
                  eps: float = 1e-5) -> T:
    """x1 = x + proj(att) + c2 * c2_scale; return x1 + fc2(GELU(fc1(LayerNorm(x1)))) in one launch (bf16x3); pk from
    prep.pack_token_projmlp.  c2_scale [K] (or [1,K]): one gate for every row.  c2_scale [B,K] with B = x.shape[0] > 1: one gate per image
    (ff_token_projmlp_images; every image must be a multiple of 256 rows), bit-equal to B calls on the row slices."""
    att_bf16 = att.dtype == torch.bfloat16
    c2_bf16 = c2 is not None and c2.dtype == torch.bfloat16
    if (att_bf16 or c2_bf16) and _GEMM_MODE != "bf16":
        raise _lib.FFError("token_projmlp: bf16 att / c2 rows exist for the plain-bf16 contraction mode only")
    ap, lda, rows, K = rows_view(att, "token_projmlp.att|bf16ok" if att_bf16 else "token_projmlp.att")
    xp, ldx, xr, xk = rows_view(x, "token_projmlp.x")
    if xr != rows or xk != K or K != pk["mlp"]["K"]:
        raise _lib.FFError("token_projmlp: shape mismatch")
    cp, ldc = None, 0
    if c2 is not None:
        cp, ldc, cr, ck = rows_view(c2, "token_projmlp.c2|bf16ok" if c2_bf16 else "token_projmlp.c2")
        if cr != rows or ck != K or c2_scale is None:
            raise _lib.FFError("token_projmlp: c2 shape mismatch")
    nimg = 1
    if c2 is not None and c2_scale.numel() != K:
        nimg = int(x.shape[0])
        if c2_scale.dim() != 2 or tuple(c2_scale.shape) != (nimg, K) or not c2_scale.is_contiguous() or rows % nimg:
            raise _lib.FFError(f"token_projmlp: c2_scale must be [{K}] or one row per image [{nimg},{K}], got {tuple(c2_scale.shape)}")
        if (rows // nimg) % 256:
            raise _lib.FFError(f"token_projmlp: a per-image gate needs images of a multiple of 256 rows, got {rows // nimg}")
    out = empty_like_rows(x)
    op_, ldo_, _, _ = rows_view(out, "token_projmlp.out")
    m = pk["mlp"]
    if nimg > 1:
        _lib.check(_L().ff_token_projmlp_images(ap, lda, xp, ldx, cp, ldc, _ptr(c2_scale), K, nimg, rows // nimg, op_, ldo_, rows, K, m["ht"],
                                                pk["proj"]["w"].data_ptr(), pk["proj"]["b"].data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                float(eps), m["w"].data_ptr(), m["b1"].data_ptr(), m["b2"].data_ptr(), _nterms(),
                                                (1 if att_bf16 else 0) | (2 if c2_bf16 else 0), _stream()))
    else:
        _lib.check(_L().ff_token_projmlp(ap, lda, xp, ldx, cp, ldc, _ptr(c2_scale), op_, ldo_, rows, K, m["ht"], pk["proj"]["w"].data_ptr(),
                                         pk["proj"]["b"].data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), m["w"].data_ptr(),
                                         m["b1"].data_ptr(), m["b2"].data_ptr(), _nterms(), (1 if att_bf16 else 0) | (2 if c2_bf16 else 0), _stream()))
    _note(2.0 * rows * K * K + 4.0 * rows * K * m["ht"] * 32, 4.0 * rows * K * (2 + (0.5 if att_bf16 else 1.0) + (0 if c2 is None else (0.5 if c2_bf16 else 1.0))))
    return out


def hab_link(att: T, x: T, pk: dict, gamma2: T, beta2: T, *, c2: T, c2_scale: T, wf: dict, rel_padded: T, gamma1: T, beta1: T,
             shift: Tuple[int, int], use_mask: bool, eps2: float = 1e-5, eps1: float = 1e-5) -> Tuple[T, T, T]:
    """One HAB's token_projmlp and the next HAB's win_attn_fused in one launch (csrc/hab_link.hip; plain bf16, 16x16 windows, six
    heads of 30): x_out = token_projmlp(att, x, pk, gamma2, beta2, c2=c2, c2_scale=c2_scale), then LayerNorm(gamma1, beta1) + qkv (wf,
    from prep.pack_win_attn) + window attention (rel_padded from prep.pack_win_rel) on x_out, which the attention takes from LDS
    instead of reading it back.  att / c2 [B,H,W,180] bf16 rows, x [B,H,W,180] fp32; c2_scale [180] (B == 1) or [B,180].
    -> (x_out fp32, xn bf16, att_out bf16), each bit-equal to the two launches."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("hab_link exists for the plain-bf16 contraction mode only")
    if att.dtype != torch.bfloat16 or c2 is None or c2.dtype != torch.bfloat16 or c2_scale is None:
        raise _lib.FFError("hab_link: att and c2 must be bf16 rows, and the gate is required")
    ap, lda, B, H, W, K = _nhwc(att, "hab_link.att|bf16ok")
    xp, ldx, xb, xh_, xw, xk = _nhwc(x, "hab_link.x")
    cp, ldc, cb, ch, cw, ck = _nhwc(c2, "hab_link.c2|bf16ok")
    if (xb, xh_, xw, xk) != (B, H, W, K) or (cb, ch, cw, ck) != (B, H, W, K) or K != pk["mlp"]["K"] or K != wf["K"]:
        raise _lib.FFError("hab_link: shape mismatch")
    if tuple(c2_scale.shape) not in (((K,), (1, K)) if B == 1 else ((B, K),)) or not c2_scale.is_contiguous():
        raise _lib.FFError(f"hab_link: c2_scale must be [{K}] for one image or one row per image [{B},{K}], got {tuple(c2_scale.shape)}")
    if tuple(rel_padded.shape[:2]) != (wf["heads"], 31) or not rel_padded.is_contiguous():
        raise _lib.FFError("hab_link: rel_padded must be [heads][31][stride]")
    out = empty_like_rows(x)
    op_, ldo_, *_ = _nhwc(out, "hab_link.out")
    xn = empty_rows_bf16(tuple(x.shape), x.device)
    xnp, ldxn, *_ = _nhwc(xn, "hab_link.xn|bf16ok")
    ao = empty_rows_bf16(tuple(x.shape), x.device)
    aop, ldao, *_ = _nhwc(ao, "hab_link.att_out|bf16ok")
    m = pk["mlp"]
    _lib.check(_L().ff_hab_link(ap, lda, xp, ldx, cp, ldc, _ptr(c2_scale), K, B, H * W, op_, ldo_, B * H * W, K, m["ht"],
                                pk["proj"]["w"].data_ptr(), pk["proj"]["b"].data_ptr(), gamma2.data_ptr(), beta2.data_ptr(), float(eps2),
                                m["w"].data_ptr(), m["b1"].data_ptr(), m["b2"].data_ptr(), 1, 3,
                                aop, ldao, 0, gamma1.data_ptr(), beta1.data_ptr(), float(eps1), wf["w"].data_ptr(), wf["b"].data_ptr(),
                                rel_padded.data_ptr(), rel_padded.shape[1], rel_padded.shape[2], H, W, 16, 16, shift[0], shift[1],
                                int(use_mask), wf["heads"], wf["d"], xnp, ldxn, 1, 1, _stream()))
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
    ld = x.stride(2)
    rows_ok = x.stride(3) == 1 and x.stride(1) == W * ld and (B == 1 or x.stride(0) == H * W * ld)
    return rows_ok and ld % 8 == 0 and ld >= C and x.data_ptr() % 16 == 0 and B * H * W * max(ld, 192) < 2 ** 31


def cab_fused(xn: T, cab0: Tuple[T, T], cab2: Tuple[T, T], out: Optional[T] = None):
    """HAT's CAB without its gate in one launch (csrc/cab_fused.hip; plain bf16): c2 = conv3x3(gelu(conv3x3(xn) + b0)) + b2 with c1 kept in
    LDS.  xn [B,H,W,180] bf16 rows; cab0 = (packed weight [60, 9*180], bias), cab2 = (packed weight [180, 9*60], bias), the pairs conv2d
    takes.  -> (c2 bf16 rows, PoolPartials), bit for bit what conv2d(xn, *cab0, act="gelu", out_bf16=True, per_image=True) followed by
    conv2d(c1, *cab2, want_pool="partials", out_bf16=True) return: the same weight images (prep.pack_conv3x3_halo, kinds "halo1"), the
    same MFMA order, and image b's partial rows are those of its own B == 1 call."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("cab_fused exists for the plain-bf16 contraction mode only")
    if xn.dtype != torch.bfloat16:
        raise _lib.FFError("cab_fused: xn must be bf16 rows")
    from . import prep as _prep
    xp, ldi, B, H, W, Cin = _nhwc(xn, "cab_fused.xn|bf16ok")
    (w0, b0), (w2, b2) = cab0, cab2
    Cmid, Cout = w0.shape[0], w2.shape[0]
    if w0.dim() != 2 or w0.shape[1] != 9 * Cin or w2.dim() != 2 or w2.shape[1] != 9 * Cmid or b0 is None or b2 is None:
        raise _lib.FFError(f"cab_fused: packed weights must be [Cmid, {9 * Cin}] and [Cout, 9 * Cmid], both with a bias")
    img0 = PREPARED.get(w0, "halo1", lambda: (_prep.pack_conv3x3_halo(w0, Cin, _prep.halo_bn(Cmid), 1), _prep.halo_bn(Cmid)))
    img2 = PREPARED.get(w2, "halo1", lambda: (_prep.pack_conv3x3_halo(w2, Cmid, _prep.halo_bn(Cout), 1), _prep.halo_bn(Cout)))
    if (img0[1], img2[1]) != (64, 192):
        raise _lib.FFError(f"cab_fused: weight images of tile widths {img0[1]} / {img2[1]}, built for 64 / 192")
    oshape = (B, H, W, Cout)
    if out is None:
        out = empty_rows_bf16(oshape, xn.device)
    elif tuple(out.shape) != oshape or out.dtype != torch.bfloat16:
        raise _lib.FFError(f"cab_fused: out must be bf16 rows {oshape}")
    op, ldo, *_ = _nhwc(out, "cab_fused.out|bf16ok")
    prow = int(_L().ff_conv3x3_halo_images_pool_rows(B, H, W, Cout, 192, 1))
    if prow < 0:
        raise _lib.FFError("cab_fused: bad shape")
    part = torch.empty((prow, 192), device=xn.device, dtype=torch.float32)
    _lib.check(_L().ff_cab_fused(xp, ldi, img0[0].data_ptr(), img0[0].numel() * img0[0].element_size(), _ptr(b0),
                                 img2[0].data_ptr(), img2[0].numel() * img2[0].element_size(), _ptr(b2), op, ldo, part.data_ptr(),
                                 B, H, W, Cin, Cmid, Cout, 1, 3, _stream()))
    _note(2.0 * B * H * W * 9 * (Cin * Cmid + Cmid * Cout), 2.0 * _numel(xn, out) + 2.0 * _numel(w0, w2))
    return out, PoolPartials(part, Cout, 1.0 / float(H * W), images=B)


def token_linear(x: T, pk: dict, *, gamma: Optional[T] = None, beta: Optional[T] = None, eps: float = 1e-5, act=None,
                 res: Optional[T] = None, res2: Optional[T] = None, res2_scale: Optional[T] = None, want_xn: bool = False,
                 stats_range: Optional[Tuple[int, int]] = None, stats_eps: float = 1e-5):
    """res + res2*scale + act(LayerNorm?(x) @ W^T + b) for K <= 192 in one launch (bf16x3); pk from prep.pack_token_linear.
    want_xn: also return LayerNorm(x) (written by the same launch) -> (out, xn).
    stats_range=(lo, hi): also return [rows, 2] (mean, rstd) of the activated output channels [lo, hi) -> (out, stats)."""
    xp, ldx, rows, K = rows_view(x, "token_linear.x")
    if K != pk["K"]:
        raise _lib.FFError("token_linear: K mismatch")
    N = pk["N"]
    # the padded row pitch of empty_rows makes every 32-column store segment of the kernel one whole 128-byte line (no
    # partial-line writes); consumers take the pitch as their ld argument
    out = empty_rows(tuple(x.shape[:-1]) + (N,), x.device)
    op, ldo, _, _ = rows_view(out, "token_linear.out")
    rp, ldr, r2p, ldr2 = None, 0, None, 0
    if res is not None:
        rp, ldr, rr, rc = rows_view(res, "token_linear.res")
        if rr != rows or rc != N:
            raise _lib.FFError("token_linear: res shape mismatch")
    if res2 is not None:
        r2p, ldr2, rr, rc = rows_view(res2, "token_linear.res2")
        if rr != rows or rc != N or res2_scale is None or res2_scale.numel() != N:
            raise _lib.FFError("token_linear: res2 shape mismatch")
    xn, xnp, ldxn = None, None, 0
    if want_xn:
        if gamma is None:
            raise _lib.FFError("token_linear: want_xn needs LayerNorm parameters")
        xn = empty_like_rows(x)
        xnp, ldxn, _, _ = rows_view(xn, "token_linear.xn")
    stats, sp, slo, shi = None, None, 0, 0
    if stats_range is not None:
        slo, shi = stats_range
        stats = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
        sp = stats.data_ptr()
    _lib.check(_L().ff_token_linear(xp, ldx, op, ldo, rows, K, pk["kpad"], N, pk["nt"], _ptr(gamma), _ptr(beta), float(eps),
                                    pk["w"].data_ptr(), _ptr(pk["b"]), ACT[act], rp, ldr, r2p, ldr2, _ptr(res2_scale), xnp, ldxn,
                                    sp, slo, shi, float(stats_eps), _nterms(), _stream()))
    _note(2.0 * rows * N * K, 4.0 * (rows * K * (2 if want_xn else 1) + rows * N * (1 + (res is not None) + (res2 is not None))))
    if stats is not None:
        return out, stats
    return (out, xn) if want_xn else out


def token_linear_rows16(x: T, pk: dict, *, gamma: Optional[T] = None, beta: Optional[T] = None, eps: float = 1e-5,
                        out: Optional[T] = None) -> T:
    """bf16( (LayerNorm?(x) @ W^T + b) * pk["scale"] ) as bf16 rows in one launch (plain bf16 only; csrc/token_linear.hip); pk from
    prep.pack_ocab_qkv.  out (optional): a bf16 rows view [..., N] to write into."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("token_linear_rows16 exists for the plain-bf16 contraction mode only")
    xp, ldx, rows, K = rows_view(x, "token_linear_rows16.x")
    if K != pk["K"]:
        raise _lib.FFError("token_linear_rows16: K mismatch")
    N = pk["N"]
    if out is None:
        out = empty_rows_bf16(tuple(x.shape[:-1]) + (N,), x.device)
    op, ldo, orows, oc = rows_view(out, "token_linear_rows16.out|bf16ok")
    if out.dtype != torch.bfloat16 or orows != rows or oc != N:
        raise _lib.FFError("token_linear_rows16: out must be bf16 rows [rows, N]")
    _lib.check(_L().ff_token_linear_rows16(xp, ldx, op, ldo, rows, K, pk["kpad"], N, pk["nt"], _ptr(gamma), _ptr(beta), float(eps),
                                           pk["w"].data_ptr(), _ptr(pk["b"]), pk["scale"].data_ptr(), ACT[None], None, 0, None, 0, None,
                                           None, 0, None, 0, 0, 0.0, 1, _stream()))
    _note(2.0 * rows * N * K, 4.0 * rows * K + 2.0 * rows * N)
    return out


def dwconv3_gate_pool(t: T, w_tap: T, bias: T):
    """t [B,H,W,2C] -> (dw3x3(t)[..., :C] * dw3x3(t)[..., C:], its per-channel mean [B,C]) in one pass.  B > 1: one launch for the
    batch (ff_dwconv3_gate_pool_images), every image with the bits of its own B == 1 call."""
    tp, ldi, B, H, W, C2 = _nhwc(t, "dwconv3_gate_pool.t")
    if B < 1 or C2 % 2 or tuple(w_tap.shape) != (9, C2):
        raise _lib.FFError("dwconv3_gate_pool: expects [B,H,W,2C] with B >= 1, [9, 2C] tap-major weights")
    C = C2 // 2
    out = torch.empty((B, H, W, C), device=t.device, dtype=torch.float32)
    pooled = torch.empty((B, C), device=t.device, dtype=torch.float32)
    if B == 1:
        nwork = int(_L().ff_dwconv3_gate_pool_workspace(C))
        work = torch.empty(nwork, device=t.device, dtype=torch.float32)
        _lib.check(_L().ff_dwconv3_gate_pool(tp, ldi, out.data_ptr(), C, H, W, C, w_tap.data_ptr(), bias.data_ptr(), pooled.data_ptr(),
                                             work.data_ptr(), nwork, _stream()))
    else:
        nwork = int(_L().ff_dwconv3_gate_pool_images_workspace(B, C))
        work = torch.empty(nwork, device=t.device, dtype=torch.float32)
        _lib.check(_L().ff_dwconv3_gate_pool_images(tp, ldi, out.data_ptr(), C, B, H, W, C, w_tap.data_ptr(), bias.data_ptr(),
                                                    pooled.data_ptr(), work.data_ptr(), nwork, _stream()))
    _note(2.0 * B * H * W * C2 * 9, 4.0 * B * H * W * (C2 + C))
    return out, pooled


def naf_front(x: T, pk: dict, ln_g: T, ln_b: T, w_tap: T, dw_bias: T, eps: float = 1e-6):
    """x [B,H,W,C] (C = 64 / 128) -> (SimpleGate(dw3x3(conv1(LayerNorm2d(x)))) [B,H,W,C], its per-channel mean [B,C]) in one launch;
    pk = prep.pack_token_linear(conv1 weight [2C, C], bias), w_tap [9, 2C] tap-major depth-wise weights.  B > 1: one launch for
    the batch (ff_naf_front_images), every image with the bits of its own B == 1 call."""
    xp, ldx, B, H, W, C = _nhwc(x, "naf_front.x")
    if B < 1 or C not in (64, 128) or pk["N"] != 2 * C or pk["K"] != C or pk["kpad"] != C or tuple(w_tap.shape) != (9, 2 * C):
        raise _lib.FFError("naf_front: expects [B,H,W,C] with B >= 1, C in (64, 128), conv1 packed as [2C, C], [9, 2C] tap-major weights")
    out = torch.empty((B, H, W, C), device=x.device, dtype=torch.float32)
    pooled = torch.empty((B, C), device=x.device, dtype=torch.float32)
    if B == 1:
        nwork = int(_L().ff_naf_front_workspace(H, W, C))
        work = torch.empty(nwork, device=x.device, dtype=torch.float32)
        _lib.check(_L().ff_naf_front(xp, ldx, H, W, C, ln_g.data_ptr(), ln_b.data_ptr(), float(eps), pk["w"].data_ptr(), pk["b"].data_ptr(),
                                     w_tap.data_ptr(), dw_bias.data_ptr(), out.data_ptr(), C, pooled.data_ptr(), work.data_ptr(), nwork,
                                     _nterms(), _stream()))
    else:
        nwork = int(_L().ff_naf_front_images_workspace(B, H, W, C))
        work = torch.empty(nwork, device=x.device, dtype=torch.float32)
        _lib.check(_L().ff_naf_front_images(xp, ldx, B, H, W, C, ln_g.data_ptr(), ln_b.data_ptr(), float(eps), pk["w"].data_ptr(),
                                            pk["b"].data_ptr(), w_tap.data_ptr(), dw_bias.data_ptr(), out.data_ptr(), C, pooled.data_ptr(),
                                            work.data_ptr(), nwork, _nterms(), _stream()))
    _note(2.0 * B * H * W * 2 * C * (C + 9), 4.0 * B * H * W * 2 * C)
    return out, pooled


def _dense_out(out: Optional[T], like: T, name: str) -> T:
    """A fresh dense fp32 tensor of like's shape, or the caller's `out` when it is one (e.g. a leading slice of a batch's buffer)."""
    if out is None:
        return torch.empty(tuple(like.shape), device=like.device, dtype=torch.float32)
    _chk(out, name + ".out")
    if tuple(out.shape) != tuple(like.shape) or not out.is_contiguous():
        raise _lib.FFError(f"{name}: out must be a contiguous float32 tensor of shape {tuple(like.shape)}")
    return out


def naf_ffn(y: T, pk: dict, ln_g: T, ln_b: T, out_scale: T, eps: float = 1e-6, out: Optional[T] = None) -> T:
    """y + out_scale * conv5(SimpleGate(conv4(LayerNorm(y)))) in one launch (C = 64 / 128, bf16x3)."""
    yp, ldy, rows, C = rows_view(y, "naf_ffn.y")
    if C != pk["C"]:
        raise _lib.FFError("naf_ffn: channel mismatch")
    out = _dense_out(out, y, "naf_ffn")
    _lib.check(_L().ff_naf_ffn(yp, ldy, out.data_ptr(), C, rows, C, ln_g.data_ptr(), ln_b.data_ptr(), float(eps), pk["w"].data_ptr(),
                               pk["b4"].data_ptr(), pk["b5"].data_ptr(), out_scale.data_ptr(), _nterms(), _stream()))
    _note(2.0 * rows * C * 3 * C, 8.0 * rows * C)
    return out


def naf_tail(g: T, x: T, pk: dict, sca: T, beta: T, ln_g: T, ln_b: T, gamma: T, eps: float = 1e-6, out: Optional[T] = None) -> T:
    """The NAFBlock tail in one launch (C = 64 / 128, plain bf16 only): y = x + beta * conv3(g * sca), then
    y + gamma * conv5(SimpleGate(conv4(LayerNorm(y)))); bit-equal to linear(g, W3, b3, res=x, mul=beta, kmul=sca) followed by
    naf_ffn.  g, x: rows views; pk from prep.pack_naf_tail.  sca [B,C] with g.shape[0] == B > 1: the rows are B equal groups, image b's
    scaled by sca[b], in one launch (ff_naf_tail_images; every image with the bits of its own call)."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError(f"naf_tail exists for the plain-bf16 contraction mode only, not {_GEMM_MODE!r}")
    gp, ldg, rows, C = rows_view(g, "naf_tail.g")
    xp, ldx, xr, xc = rows_view(x, "naf_tail.x")
    if C != pk["C"] or xr != rows or xc != C or tuple(x.shape) != tuple(g.shape):
        raise _lib.FFError("naf_tail: shape mismatch")
    images = sca.shape[0] if isinstance(sca, torch.Tensor) and sca.dim() == 2 and sca.shape[0] > 1 else 1
    if images > 1:
        _chk(sca, "naf_tail.sca")
        if g.dim() < 2 or g.shape[0] != images or tuple(sca.shape) != (images, C) or not sca.is_contiguous():
            raise _lib.FFError(f"naf_tail: sca {tuple(sca.shape)} must be a contiguous [B, {C}] matrix with B the leading dimension of g {tuple(g.shape)}")
    for t_, n_ in ((beta, "beta"), (ln_g, "ln_g"), (ln_b, "ln_b"), (gamma, "gamma")) + (() if images > 1 else ((sca, "sca"),)):
        _chk(t_, "naf_tail." + n_)
        if t_.numel() != C or not t_.is_contiguous():
            raise _lib.FFError(f"naf_tail: {n_} must be a contiguous [{C}] vector")
    out = _dense_out(out, x, "naf_tail")
    if images > 1:
        _lib.check(_L().ff_naf_tail_images(gp, ldg, xp, ldx, out.data_ptr(), C, rows, C, sca.data_ptr(), images, rows // images,
                                           pk["b3"].data_ptr(), beta.data_ptr(), ln_g.data_ptr(), ln_b.data_ptr(), float(eps),
                                           pk["w"].data_ptr(), pk["b4"].data_ptr(), pk["b5"].data_ptr(), gamma.data_ptr(), _stream()))
    else:
        _lib.check(_L().ff_naf_tail(gp, ldg, xp, ldx, out.data_ptr(), C, rows, C, sca.data_ptr(), pk["b3"].data_ptr(), beta.data_ptr(),
                                    ln_g.data_ptr(), ln_b.data_ptr(), float(eps), pk["w"].data_ptr(), pk["b4"].data_ptr(),
                                    pk["b5"].data_ptr(), gamma.data_ptr(), _stream()))
    _note(2.0 * rows * C * 4 * C, 12.0 * rows * C)
    return out


def layernorm(x: T, gamma: T, beta: T, eps: float = 1e-5, out: Optional[T] = None, out_bf16: bool = False) -> T:
    """out_bf16: bf16 output rows, (bf16) of the fp32 result, for a consumer that rounds them to bf16 anyway."""
    xp, ldi, rows, C = rows_view(x, "layernorm.x")
    if out is None:
        out = empty_rows_bf16(tuple(x.shape), x.device) if out_bf16 else empty_like_rows(x)
    elif (out.dtype == torch.bfloat16) != out_bf16:
        raise _lib.FFError("layernorm: out dtype does not match out_bf16")
    op, ldo, orows, oc = rows_view(out, "layernorm.out|bf16ok" if out_bf16 else "layernorm.out")
    if orows != rows or oc != C or gamma.numel() != C or beta.numel() != C:
        raise _lib.FFError("layernorm: shape mismatch")
    fn = _L().ff_layernorm_bf16out if out_bf16 else _L().ff_layernorm
    _lib.check(fn(xp, ldi, op, ldo, rows, C, gamma.data_ptr(), beta.data_ptr(), float(eps), _stream()))
    _note(0.0, (6.0 if out_bf16 else 8.0) * rows * C)
    return out


def pool_partials(x: T):
    """First stage of the global average pool of x [B,H,W,C] -> PoolPartials (vec_mlp finishes them in its own launch).  B > 1: one
    launch for the batch (ff_pool_partials_images; H * W a multiple of 256), PoolPartials(images=B) holding image b's rows as its own
    B == 1 call writes them."""
    xp, ld, B, H, W, C = _nhwc(x, "pool_partials.x")
    P = H * W
    if B != 1:
        if B < 1 or P % 256:
            raise _lib.FFError(f"pool_partials: a batch needs images of a multiple of 256 pixels, got {tuple(x.shape)}")
        rows = int(_L().ff_pool_partials_images_rows(B, P))
        part = torch.empty((rows, C), device=x.device, dtype=torch.float32)
        _lib.check(_L().ff_pool_partials_images(xp, ld, B, P, C, part.data_ptr(), part.numel(), _stream()))
        return PoolPartials(part, C, 1.0 / float(P), images=B)
    rows = int(_L().ff_pool_partial_rows(P))
    part = torch.empty((rows, C), device=x.device, dtype=torch.float32)
    _lib.check(_L().ff_pool_partials(xp, ld, P, C, part.data_ptr(), part.numel(), _stream()))
    return PoolPartials(part, C, 1.0 / float(P))


def pool_mean(x: T) -> T:
    """[B,H,W,C] rows view -> [B,C]."""
    xp, ld, B, H, W, C = _nhwc(x, "pool_mean.x")
    P = H * W
    nwork = int(_L().ff_pool_mean_workspace(B, P, C))
    work = torch.empty(nwork, device=x.device, dtype=torch.float32)
    out = torch.empty((B, C), device=x.device, dtype=torch.float32)
    _lib.check(_L().ff_pool_mean(xp, ld, B, P, C, out.data_ptr(), work.data_ptr(), nwork, _stream()))
    _note(0.0, 4.0 * B * P * C)
    return out


def vec_mlp(v, W1: T, b1: Optional[T], act1, W2: Optional[T] = None, b2: Optional[T] = None, act2=None,
            post: float = 1.0) -> T:
    """act2(W2 . act1(W1 . v + b1) + b2) * post per row of v [B, Cin] (W2 None: one layer).  v may be a PoolPartials: the pool is
    then finished inside the same launch (two-layer form with a hidden width <= 64), otherwise finished first."""
    if isinstance(v, PoolPartials):
        if W2 is not None and W1.shape[0] <= 64 and v.C <= 512:
            if W1.shape[1] != v.C or W2.shape[1] != W1.shape[0]:
                raise _lib.FFError("vec_mlp: weight shape mismatch")
            out = torch.empty((v.images, W2.shape[0]), device=v.part.device, dtype=torch.float32)
            if v.images > 1:                                 # one workgroup per image, each in the single-image summation order
                _lib.check(_L().ff_pool_vec_mlp_images(v.part.data_ptr(), v.images, v.rows_per_image, v.part.shape[1], v.inv_count, v.C,
                                                       W1.data_ptr(), _ptr(b1), W1.shape[0], ACT[act1], W2.data_ptr(), _ptr(b2), W2.shape[0],
                                                       ACT[act2], float(post), out.data_ptr(), None, _stream()))
                return out
            _lib.check(_L().ff_pool_vec_mlp(v.part.data_ptr(), v.part.shape[0], v.part.shape[1], v.inv_count, v.C, W1.data_ptr(), _ptr(b1),
                                            W1.shape[0], ACT[act1], W2.data_ptr(), _ptr(b2), W2.shape[0], ACT[act2], float(post),
                                            out.data_ptr(), None, _stream()))
            return out
        v = v.mean()
    B, Cin = v.shape
    Ch = W1.shape[0]
    Cout = W2.shape[0] if W2 is not None else Ch
    if W1.shape[1] != Cin or (W2 is not None and W2.shape[1] != Ch):
        raise _lib.FFError("vec_mlp: weight shape mismatch")
    out = torch.empty((B, Cout), device=v.device, dtype=torch.float32)
    _lib.check(_L().ff_vec_mlp(v.data_ptr(), B, Cin, W1.data_ptr(), _ptr(b1), Ch, ACT[act1], _ptr(W2), _ptr(b2), Cout,
                               ACT[act2], float(post), out.data_ptr(), _stream()))
    return out


def pixel_mlp(x: T, W1: T, b1: Optional[T], act1, w2: T, b2: float, act2) -> T:
    """[..., C] rows -> [..., 1]: act2(w2 . act1(W1 x + b1) + b2) per row, hidden width <= 16 (fp32, one launch)."""
    xp, ldi, rows, C = rows_view(x, "pixel_mlp.x")
    Hd = W1.shape[0]
    if tuple(W1.shape) != (Hd, C) or w2.numel() != Hd or not W1.is_contiguous():
        raise _lib.FFError("pixel_mlp: weight shape mismatch")
    out = torch.empty(tuple(x.shape[:-1]) + (1,), device=x.device, dtype=torch.float32)
    _lib.check(_L().ff_pixel_mlp(xp, ldi, rows, C, Hd, W1.data_ptr(), _ptr(b1), ACT[act1], w2.reshape(-1).data_ptr(), float(b2), ACT[act2],
                                 out.data_ptr(), _stream()))
    _note(2.0 * rows * C * Hd, 4.0 * rows * (C + 1))
    return out


def dwconv2d(x: T, w_tap: T, bias: Optional[T] = None, *, ksize=(3, 3), stride=(1, 1), pad=(1, 1),
             post_scale: Optional[T] = None, post_shift: Optional[T] = None, act=None, out: Optional[T] = None,
             mul_in: Optional[T] = None) -> T:
    xp, ldi, B, H, W, C = _nhwc(x, "dwconv2d.x")
    KH, KW = ksize
    if tuple(w_tap.shape) != (KH * KW, C) or not w_tap.is_contiguous():
        raise _lib.FFError(f"dwconv2d: tap-major weight must be [{KH * KW},{C}]")
    Ho = (H + 2 * pad[0] - KH) // stride[0] + 1
    Wo = (W + 2 * pad[1] - KW) // stride[1] + 1
    if out is None:
        out = empty_rows((B, Ho, Wo, C), x.device)
    op, ldo, *_ = _nhwc(out, "dwconv2d.out")
    mp, ldm = None, 0
    if mul_in is not None:
        mp, ldm, mb, mh, mw, mc = _nhwc(mul_in, "dwconv2d.mul_in")
        if (mb, mh, mw, mc) != (B, Ho, Wo, C):
            raise _lib.FFError("dwconv2d: mul_in shape mismatch")
    _lib.check(_L().ff_dwconv2d(xp, ldi, op, ldo, B, H, W, C, Ho, Wo, w_tap.data_ptr(), _ptr(bias), KH, KW, stride[0],
                                stride[1], pad[0], pad[1], _ptr(post_scale), _ptr(post_shift), ACT[act], mp, ldm, _stream()))
    _note(2.0 * B * Ho * Wo * C * KH * KW, 4.0 * (B * H * W * C + B * Ho * Wo * C))
    return out


def token_linear_gated(x: T, x2: T, pk: dict, cm: T, gb2: float, *, res: Optional[T] = None) -> T:
    """res + W (x * cm[channel] + x2 * sm[token]) + b with sm = sigmoid(gw2 . gelu(GW1 x + gb1) + gb2) in one launch (bf16x3);
    pk from prep.pack_token_linear_gated.  cm [K] (or [1,K]): one channel gate for every row.  cm [B,K] with B > 1: the rows are B images of
    a multiple of 256 rows each, image b gated by cm[b], in one launch (ff_token_linear_gated_images) -- bit-equal to B calls."""
    xp, ldx, rows, K = rows_view(x, "token_linear_gated.x")
    x2p, ldx2, r2, k2 = rows_view(x2, "token_linear_gated.x2")
    _chk(cm, "token_linear_gated.cm")
    if r2 != rows or k2 != K or K != pk["K"]:
        raise _lib.FFError("token_linear_gated: shape mismatch")
    images = 1
    if cm.numel() != K:                                      # (refusals first: nothing is launched before them)
        if cm.dim() != 2 or cm.shape[1] != K or cm.shape[0] < 1 or not cm.is_contiguous():
            raise _lib.FFError(f"token_linear_gated: cm must be [{K}] or one contiguous row per image [B,{K}], got {tuple(cm.shape)}")
        images = int(cm.shape[0])
        if rows % images or (rows // images) % 256:
            raise _lib.FFError(f"token_linear_gated: a per-image gate needs B = {images} images of a multiple of 256 rows, got {rows} rows")
    N = pk["N"]
    out = empty_rows(tuple(x.shape[:-1]) + (N,), x.device)
    op, ldo, _, _ = rows_view(out, "token_linear_gated.out")
    rp, ldr = None, 0
    if res is not None:
        rp, ldr, rr, rc = rows_view(res, "token_linear_gated.res")
        if rr != rows or rc != N:
            raise _lib.FFError("token_linear_gated: res shape mismatch")
    if images > 1:
        _lib.check(_L().ff_token_linear_gated_images(xp, ldx, x2p, ldx2, cm.data_ptr(), images, rows // images, pk["gb1"].data_ptr(),
                                                     pk["gw2"].data_ptr(), float(gb2), op, ldo, rows, K, N, pk["nt"], pk["w"].data_ptr(),
                                                     pk["b"].data_ptr(), rp, ldr, _nterms(), _stream()))
    else:
        _lib.check(_L().ff_token_linear_gated(xp, ldx, x2p, ldx2, cm.data_ptr(), None, pk["gb1"].data_ptr(), pk["gw2"].data_ptr(), float(gb2),
                                              op, ldo, rows, K, N, pk["nt"], pk["w"].data_ptr(), pk["b"].data_ptr(), rp, ldr, _nterms(), _stream()))
    _note(2.0 * rows * N * K + 2.0 * rows * 32 * K, 4.0 * rows * (2 * K + N * (2 if res is not None else 1)))
    return out


def dwconv3x3_ln(x: T, w_tap: T, bias: Optional[T], stats: T, gamma: T, beta: T, mul_in: Optional[T] = None) -> T:
    """(dw3x3(LayerNorm(x)) + bias) * mul_in with the LayerNorm applied on load from per-token (mean, rstd) `stats`."""
    xp, ldi, B, H, W, C = _nhwc(x, "dwconv3x3_ln.x")
    if tuple(w_tap.shape) != (9, C) or tuple(stats.shape) != (B * H * W, 2) or gamma.numel() != C or beta.numel() != C:
        raise _lib.FFError("dwconv3x3_ln: shape mismatch")
    out = empty_rows((B, H, W, C), x.device)
    op, ldo, *_ = _nhwc(out, "dwconv3x3_ln.out")
    mp, ldm = None, 0
    if mul_in is not None:
        mp, ldm, mb, mh, mw, mc = _nhwc(mul_in, "dwconv3x3_ln.mul_in")
        if (mb, mh, mw, mc) != (B, H, W, C):
            raise _lib.FFError("dwconv3x3_ln: mul_in shape mismatch")
    _lib.check(_L().ff_dwconv3x3_ln(xp, ldi, op, ldo, B, H, W, C, w_tap.data_ptr(), _ptr(bias), stats.data_ptr(), gamma.data_ptr(),
                                    beta.data_ptr(), mp, ldm, _stream()))
    _note(2.0 * B * H * W * C * 9, 4.0 * B * H * W * C * (3 if mul_in is not None else 2))
    return out


def sgfn_tail(y: T, c2: int, w_tap: T, dw_bias: Optional[T], stats: T, gamma: T, beta: T, w2: T, b2: Optional[T], res: Optional[T] = None) -> T:
    """res + fc2(y[..., :c2] * (dw3x3(LayerNorm(y[..., c2:2 c2])) + dw_bias)) + b2 in one launch (plain bf16; csrc/sgfn_tail.hip).
    y [B,H,W,>= 2 c2] rows view (fc1's output), stats [B*H*W, 2] = (mean, rstd) of y[..., c2:], w_tap [9, c2], w2 [N, c2]."""
    if _GEMM_MODE != "bf16":
        raise _lib.FFError("sgfn_tail exists for the plain-bf16 contraction mode only")
    yp, ldh, B, H, W, Cy = _nhwc(y, "sgfn_tail.y")
    N = w2.shape[0]
    if Cy < 2 * c2 or tuple(w_tap.shape) != (9, c2) or tuple(stats.shape) != (B * H * W, 2) or gamma.numel() != c2 or beta.numel() != c2 \
            or w2.shape[1] != c2:
        raise _lib.FFError("sgfn_tail: shape mismatch")
    from . import prep as _prep
    tiles = PREPARED.get(w2, "sgfn", lambda: _prep.pack_sgfn_fc2(w2))
    out = empty_rows((B, H, W, N), y.device)
    op, ldo, *_ = _nhwc(out, "sgfn_tail.out")
    rp, ldr = None, 0
    if res is not None:
        if tuple(res.shape) != (B, H, W, N):
            raise _lib.FFError("sgfn_tail: res shape mismatch")
        rp, ldr, *_ = _nhwc(res, "sgfn_tail.res")
    _lib.check(_L().ff_sgfn_tail(yp, ldh, c2, stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w_tap.data_ptr(), _ptr(dw_bias),
                                 tiles.data_ptr(), tiles.shape[0], _ptr(b2), rp, ldr, op, ldo, B, H, W, N, _stream()))
    _note(2.0 * B * H * W * c2 * (9 + N), 4.0 * B * H * W * (2 * c2 + 2 * N))
    return out


def mix2(a: T, b: Optional[T] = None, *, ka: float = 1.0, kb: float = 1.0, ca: Optional[T] = None,
         cb: Optional[T] = None, pa: Optional[T] = None, pb: Optional[T] = None, clamp01: bool = False,
         out: Optional[T] = None) -> T:
    """out = ka*a*ca[c]*pa[p] + kb*b*cb[c]*pb[p].  ca [B, C] with B > 1: the rows are B equal groups (one image each) and group b is scaled
    by ca[b], in one launch (ff_mix2_images) -- every image with the bits of its own call with ca[b]."""
    ap, lda, rows, C = rows_view(a, "mix2.a")
    bp, ldb = None, 0
    if b is not None:
        bp, ldb, brows, bc = rows_view(b, "mix2.b")
        if brows != rows or bc != C:
            raise _lib.FFError("mix2: a/b shape mismatch")
    if out is None:
        out = empty_like_rows(a)
    op, ldo, orows, oc = rows_view(out, "mix2.out")
    if orows != rows or oc != C:
        raise _lib.FFError("mix2: out shape mismatch")

    def pvec(p, nm):
        if p is None:
            return None, 0
        pp, ldp, prows, pc = rows_view(p, nm)
        if prows != rows or pc != 1:
            raise _lib.FFError(f"{nm}: per-row vector must be [rows,1]")
        return pp, ldp

    pap, ldpa = pvec(pa, "mix2.pa")
    pbp, ldpb = pvec(pb, "mix2.pb")
    images = 1
    if ca is not None and ca.dim() == 2 and ca.shape[0] > 1:
        images = int(ca.shape[0])
        _chk(ca, "mix2.ca")
        if ca.shape[1] != C or not ca.is_contiguous() or rows % images:
            raise _lib.FFError(f"mix2: ca {tuple(ca.shape)} must be a contiguous [B, {C}] matrix with B dividing the {rows} rows")
    for v_, nm in ((ca, "ca"), (cb, "cb")):
        if v_ is not None and v_.numel() != C * (images if nm == "ca" else 1):
            raise _lib.FFError(f"mix2: {nm} must have {C} elements")
    if images > 1:
        _lib.check(_L().ff_mix2_images(op, ldo, ap, lda, bp, ldb, rows, C, float(ka), float(kb), ca.data_ptr(), images, rows // images,
                                       _ptr(cb), pap, ldpa, pbp, ldpb, int(clamp01), _stream()))
        _note(0.0, 4.0 * rows * C * (3 if b is not None else 2))
        return out
    _lib.check(_L().ff_mix2(op, ldo, ap, lda, bp, ldb, rows, C, float(ka), float(kb), _ptr(ca), _ptr(cb), pap, ldpa, pbp,
                            ldpb, int(clamp01), _stream()))
    _note(0.0, 4.0 * rows * C * (3 if b is not None else 2))
    return out


def fma3(a: Optional[T], b: T, c: T, alpha: float = 1.0, out: Optional[T] = None) -> T:
    bp, ldb, rows, C = rows_view(b, "fma3.b")
    cp, ldc, crows, cc = rows_view(c, "fma3.c")
    if crows != rows or cc != C:
        raise _lib.FFError("fma3: b/c shape mismatch")
    ap, lda = None, 0
    if a is not None:
        ap, lda, arows, ac = rows_view(a, "fma3.a")
        if arows != rows or ac != C:
            raise _lib.FFError("fma3: a shape mismatch")
    if out is None:
        out = empty_like_rows(b)
    op, ldo, orows, oc = rows_view(out, "fma3.out")
    if orows != rows or oc != C:
        raise _lib.FFError("fma3: out shape mismatch")
    _lib.check(_L().ff_fma3(op, ldo, ap, lda, bp, ldb, cp, ldc, rows, C, float(alpha), _stream()))
    _note(0.0, 4.0 * rows * C * (4 if a is not None else 3))
    return out


def affine(x: T, scale: T, shift: T, act=None, out: Optional[T] = None) -> T:
    xp, ldi, rows, C = rows_view(x, "affine.x")
    if out is None:
        out = empty_like_rows(x)
    op, ldo, orows, oc = rows_view(out, "affine.out")
    if orows != rows or oc != C or scale.numel() != C or shift.numel() != C:
        raise _lib.FFError("affine: shape mismatch")
    _lib.check(_L().ff_affine(op, ldo, xp, ldi, rows, C, scale.data_ptr(), shift.data_ptr(), ACT[act], _stream()))
    _note(0.0, 8.0 * rows * C)
    return out


def u8_to_f32_image(img_u8: T) -> T:
    """uint8 HWC [H,W,3] on the device -> fp32 [1,3,H,W] in [0,1] (reference io.py:64-68)."""
    if not (isinstance(img_u8, torch.Tensor) and img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.dim() == 3
            and img_u8.shape[2] == 3 and img_u8.is_contiguous()):
        raise _lib.FFError("u8_to_f32_image: expected a contiguous CUDA(HIP) uint8 [H,W,3] tensor")
    H, W, _ = img_u8.shape
    out = torch.empty((1, 3, H, W), device=img_u8.device, dtype=torch.float32)
    _lib.check(_L().ff_u8hwc_to_f32nchw(img_u8.data_ptr(), out.data_ptr(), H, W, _stream()))
    return out


def f32_to_u8_image(x: T) -> T:
    """fp32 [1,3,H,W] (or [3,H,W]) -> uint8 HWC [H,W,3]: clamp, *255, round half to even (reference io.py:71-76)."""
    _chk(x, "f32_to_u8_image.x")
    if x.dim() == 4:
        if x.shape[0] != 1:
            raise _lib.FFError("f32_to_u8_image: batch must be 1")
        x = x[0]
    if x.dim() != 3 or x.shape[0] != 3:
        raise _lib.FFError("f32_to_u8_image: expected [1,3,H,W] or [3,H,W]")
    x = x.contiguous()
    _, H, W = x.shape
    out = torch.empty((H, W, 3), device=x.device, dtype=torch.uint8)
    _lib.check(_L().ff_f32nchw_to_u8hwc(x.data_ptr(), out.data_ptr(), H, W, _stream()))
    return out


def nchw_to_nhwc(x: T, Hp: Optional[int] = None, Wp: Optional[int] = None, add: Optional[T] = None,
                 pad_mode: str = "zero", out: Optional[T] = None) -> T:
    _chk(x, "nchw_to_nhwc.x")
    x = x.contiguous()
    B, C, H, W = x.shape
    Hp, Wp = Hp or H, Wp or W
    if out is None:
        out = empty_rows((B, Hp, Wp, C), x.device)
    op, ldo, *_ = _nhwc(out, "nchw_to_nhwc.out")
    _lib.check(_L().ff_nchw_to_nhwc(x.data_ptr(), op, B, C, H, W, Hp, Wp, ldo, _ptr(add), 1 if pad_mode == "reflect" else 0,
                                    _stream()))
    return out


def nhwc_to_nchw(x: T, H: Optional[int] = None, W: Optional[int] = None, add: Optional[T] = None, clamp01: bool = False,
                 out: Optional[T] = None) -> T:
    xp, ldi, B, Hs, Ws, C = _nhwc(x, "nhwc_to_nchw.x")
    H, W = H or Hs, W or Ws
    if out is None:
        out = torch.empty((B, C, H, W), device=x.device, dtype=torch.float32)
    else:
        _chk(out, "nhwc_to_nchw.out")
        if tuple(out.shape) != (B, C, H, W) or not out.is_contiguous():
            raise _lib.FFError(f"nhwc_to_nchw: out must be a contiguous [{B},{C},{H},{W}] tensor")
    _lib.check(_L().ff_nhwc_to_nchw(xp, out.data_ptr(), B, C, H, W, Hs, Ws, ldi, _ptr(add), int(clamp01), _stream()))
    return out


def _aten_scale(n_in: int, n_out: int, scale_factor: Optional[float]) -> float:
    """ATen area_pixel_compute_scale (align_corners=False): 1/scale_factor if given else in/out, in fp32."""
    import numpy as np
    if scale_factor is not None and scale_factor > 0:
        return float(np.float32(1.0) / np.float32(scale_factor))
    return float(np.float32(n_in) / np.float32(n_out))


def resize(x: T, size: Tuple[int, int], *, mode: str = "bilinear", scale_factor: Optional[float] = None,
           layout: str = "nhwc", out: Optional[T] = None, mul: float = 1.0) -> T:
    """x NHWC rows view [B,H,W,C] or planar [B,C,H,W] (layout='nchw'); out is always NHWC (may be a channel slice)."""
    Ho, Wo = size
    if layout == "nhwc":
        xp, ld, B, Hi, Wi, C = _nhwc(x, "resize.x")
        isb, isc, isy, isx = Hi * Wi * ld, 1, Wi * ld, ld
    else:
        _chk(x, "resize.x")
        x = x.contiguous()
        B, C, Hi, Wi = x.shape
        xp = x.data_ptr()
        isb, isc, isy, isx = C * Hi * Wi, Hi * Wi, Wi, 1
    if out is None:
        out = torch.empty((B, Ho, Wo, C), device=x.device, dtype=torch.float32)
    op, ldo, ob, oh, ow, oc = _nhwc(out, "resize.out")      # out may be larger than (Ho, Wo): the top-left region is written
    if ob != B or oc != C or oh < Ho or ow < Wo:
        raise _lib.FFError("resize: out shape mismatch")
    sh = _aten_scale(Hi, Ho, scale_factor)
    sw = _aten_scale(Wi, Wo, scale_factor)
    _lib.check(_L().ff_resize(xp, isb, isc, isy, isx, Hi, Wi, op, oh * ow * ldo, 1, ow * ldo, ldo, Ho, Wo, B, C, sh, sw,
                              0 if mode == "bilinear" else 1, float(mul), _stream()))
    _note(0.0, 4.0 * B * C * (Hi * Wi + Ho * Wo))
    return out


def avgpool2(x: T) -> T:
    xp, ldi, B, H, W, C = _nhwc(x, "avgpool2.x")
    out = torch.empty((B, H // 2, W // 2, C), device=x.device, dtype=torch.float32)
    _lib.check(_L().ff_avgpool2(xp, ldi, out.data_ptr(), C, B, H, W, C, _stream()))
    return out


def _planar_images(x: T, out: T, name: str):
    """Planar image(s) [3,H,W] or contiguous [B,3,H,W] and their NHWC output [B,H,W,>=..] -> (B, H, W, out pointer, ldo)."""
    _chk(x, name + ".x")
    B = int(x.shape[0]) if x.dim() == 4 else 1
    C, H, W = x.shape[-3:]
    op, ldo, ob, oh, ow, _ = _nhwc(out, name + ".out")
    if B > 1 and (not x.is_contiguous() or C != 3 or (ob, oh, ow) != (B, H, W)):
        raise _lib.FFError(f"{name}: expected contiguous planar images [B,3,H,W] and out [B,H,W,.], got {tuple(x.shape)} and {tuple(out.shape)}")
    if B > 1 and out.stride(0) != H * W * ldo:
        raise _lib.FFError(f"{name}: the images of out must follow each other ([B,H,W,ld] rows)")
    return B, C, H, W, op, ldo


def dct8_bands(x_planar: T, dct_mat: T, masks3: T, band_scale: T, out: T, ch_off: int):
    """x_planar [3,H,W] (or [1,3,H,W]); [B,3,H,W] with B > 1: the batch in one launch (ff_dct8_bands_images)."""
    B, C, H, W, op, ldo = _planar_images(x_planar, out, "dct8_bands")
    if B > 1:
        _lib.check(_L().ff_dct8_bands_images(x_planar.data_ptr(), B, H, W, dct_mat.data_ptr(), masks3.data_ptr(), band_scale.data_ptr(),
                                             op, ldo, ch_off, _stream()))
        return
    _lib.check(_L().ff_dct8_bands(x_planar.data_ptr(), C, H, W, dct_mat.data_ptr(), masks3.data_ptr(), band_scale.data_ptr(),
                                  op, ldo, ch_off, _stream()))


def dwt_pass(x_planar: T, axis: int, lo8: T, hi8: T) -> Tuple[T, T]:
    _chk(x_planar, "dwt_pass.x")
    C, H, W = x_planar.shape
    Ho = (H + 6) // 2 + 1 if axis == 0 else H
    Wo = (W + 6) // 2 + 1 if axis == 1 else W
    lo = torch.empty((C, Ho, Wo), device=x_planar.device, dtype=torch.float32)
    hi = torch.empty_like(lo)
    _lib.check(_L().ff_dwt_pass(x_planar.data_ptr(), C, H, W, axis, lo8.data_ptr(), hi8.data_ptr(), lo.data_ptr(),
                                hi.data_ptr(), _stream()))
    return lo, hi


def fft_bands(x_planar: T, twW: Tuple[T, T], twH: Tuple[T, T], mask_logits: T, temp: float, band_scale2: T, out: T,
              ch_lo: int, ch_hi: int):
    B, C, H, W, op, ldo = _planar_images(x_planar, out, "fft_bands")
    msz = mask_logits.shape[-1]
    if B > 1:                                                # the batch through one run of the four kernels (ff_fft_bands_images)
        nwork = int(_L().ff_fft_bands_images_workspace(B, H, W))
        if nwork < 0:
            raise _lib.FFError(f"fft_bands: no batched form for {tuple(x_planar.shape)}")
        work = torch.empty(nwork, device=x_planar.device, dtype=torch.float32)
        _lib.check(_L().ff_fft_bands_images(x_planar.data_ptr(), B, H, W, twW[0].data_ptr(), twW[1].data_ptr(), twH[0].data_ptr(),
                                            twH[1].data_ptr(), mask_logits.data_ptr(), msz, float(temp), band_scale2.data_ptr(),
                                            work.data_ptr(), nwork, op, ldo, ch_lo, ch_hi, _stream()))
        return
    nwork = 4 * C * H * (W // 2 + 1)
    work = torch.empty(nwork, device=x_planar.device, dtype=torch.float32)
    _lib.check(_L().ff_fft_bands(x_planar.data_ptr(), C, H, W, twW[0].data_ptr(), twW[1].data_ptr(), twH[0].data_ptr(),
                                 twH[1].data_ptr(), mask_logits.data_ptr(), msz, float(temp), band_scale2.data_ptr(),
                                 work.data_ptr(), nwork, op, ldo, ch_lo, ch_hi, _stream()))


def chan_attn_weights(qkv: T, q_off: int, k_off: int, temperature: T) -> T:
    qp, ld, rows, C = rows_view(qkv, "chan_attn_weights.qkv")
    nwork = int(_L().ff_chan_attn_workspace(rows))
    work = torch.empty(nwork, device=qkv.device, dtype=torch.float32)
    wbd = torch.empty((180, 180), device=qkv.device, dtype=torch.float32)
    _lib.check(_L().ff_chan_attn_weights(qp, ld, q_off, k_off, rows, temperature.data_ptr(), wbd.data_ptr(), work.data_ptr(),
                                         nwork, _stream()))
    return wbd


def chan_qkv_attn(x: T, pk: dict, gamma: T, beta: T, temperature: T, eps: float = 1e-5):
    """DAT channel attention front end in two launches (ff_chan_qkv + ff_chan_attn_finish): x [..., 180] ->
    (v [..., 180], block-diagonal attention matrix [180, 180]); q and k never reach memory.
    x [B,H,W,180] with B > 1 (H * W a multiple of 256): still two launches -- ff_chan_qkv's partials are per 256-token workgroup, so one call
    covers the batch, and ff_chan_attn_finish_images reduces every image's own blocks in the single-image order -> wbd [B,180,180], every
    image's matrix (and v) with the bits of its own call."""
    xp, ldx, rows, K = rows_view(x, "chan_qkv_attn.x")
    if K != pk["K"]:
        raise _lib.FFError("chan_qkv_attn: K mismatch")
    images = int(x.shape[0]) if x.dim() == 4 and x.shape[0] > 1 else 1
    if images > 1:
        if (rows // images) % 256:
            raise _lib.FFError(f"chan_qkv_attn: a batch needs images of a multiple of 256 tokens, got {tuple(x.shape)}")
        v = empty_like_rows(x)
        vp, ldv, _, _ = rows_view(v, "chan_qkv_attn.v")
        nwork = int(_L().ff_chan_qkv_images_workspace(images, rows // images))
        work = torch.empty(nwork, device=x.device, dtype=torch.float32)
        wbd = torch.empty((images, 180, 180), device=x.device, dtype=torch.float32)
        _lib.check(_L().ff_chan_qkv(xp, ldx, rows, K, gamma.data_ptr(), beta.data_ptr(), float(eps), pk["w"].data_ptr(), pk["b"].data_ptr(),
                                    vp, ldv, work.data_ptr(), nwork, _nterms(), _stream()))
        _lib.check(_L().ff_chan_attn_finish_images(work.data_ptr(), nwork, images, rows // images, temperature.data_ptr(), wbd.data_ptr(),
                                                   _stream()))
        _note(2.0 * rows * 576 * K + 2.0 * rows * 6 * 32 * 32, 8.0 * rows * K)
        return v, wbd
    v = empty_like_rows(x)
    vp, ldv, _, _ = rows_view(v, "chan_qkv_attn.v")
    nwork = int(_L().ff_chan_qkv_workspace(rows))
    work = torch.empty(nwork, device=x.device, dtype=torch.float32)
    wbd = torch.empty((180, 180), device=x.device, dtype=torch.float32)
    _lib.check(_L().ff_chan_qkv(xp, ldx, rows, K, gamma.data_ptr(), beta.data_ptr(), float(eps), pk["w"].data_ptr(), pk["b"].data_ptr(),
                                vp, ldv, work.data_ptr(), nwork, _nterms(), _stream()))
    _lib.check(_L().ff_chan_attn_finish(work.data_ptr(), nwork, (rows + 255) // 256, temperature.data_ptr(), wbd.data_ptr(), _stream()))
    _note(2.0 * rows * 576 * K + 2.0 * rows * 6 * 32 * 32, 8.0 * rows * K)
    return v, wbd


def band_mha_core(qkv: T, P: int, nbands: int, heads: int) -> T:
    _chk(qkv, "band_mha_core.qkv")
    E = qkv.shape[-1] // 3
    out = torch.empty((P * nbands, E), device=qkv.device, dtype=torch.float32)
    _lib.check(_L().ff_band_mha_core(qkv.data_ptr(), out.data_ptr(), P, nbands, heads, _stream()))
    return out


def band_weight(x: T, att: T, imp: T) -> T:
    out = torch.empty_like(x)
    P = x.numel() // x.shape[-1]
    _lib.check(_L().ff_band_weight(x.data_ptr(), att.data_ptr(), imp.data_ptr(), out.data_ptr(), P, x.shape[-1] // 3, _stream()))
    return out


def freq_guidance(b3: T) -> T:
    P = b3.numel() // 9
    out = torch.empty(tuple(b3.shape[:-1]) + (3,), device=b3.device, dtype=torch.float32)
    _lib.check(_L().ff_freq_guidance(b3.data_ptr(), out.data_ptr(), P, _stream()))
    return out


def dynamic_gates(graw: T, dif: T) -> T:
    P = graw.numel() // 3
    out = torch.empty_like(graw)
    _lib.check(_L().ff_dynamic_gates(graw.data_ptr(), dif.data_ptr(), out.data_ptr(), P, _stream()))
    return out


def fuse_blend(experts9: T, hier3: T, guide3: T, gates3: T, dif1: T) -> T:
    """experts9 [B,Hh,Wh,9], hier3 [B,Hh,Wh,3], guide3 / gates3 [B,Hl,Wl,3], dif1 [B,Hl,Wl,1], all contiguous -> [B,Hh,Wh,3]; B > 1 in one
    launch (ff_fuse_blend_images)."""
    B, Hh, Wh, _ = experts9.shape
    _, Hl, Wl, _ = guide3.shape
    out = torch.empty((B, Hh, Wh, 3), device=experts9.device, dtype=torch.float32)
    if B > 1:
        for t, c, hw in ((experts9, 9, (Hh, Wh)), (hier3, 3, (Hh, Wh)), (guide3, 3, (Hl, Wl)), (gates3, 3, (Hl, Wl)), (dif1, 1, (Hl, Wl))):
            _chk(t, "fuse_blend")
            if tuple(t.shape) != (B, *hw, c) or not t.is_contiguous():
                raise _lib.FFError(f"fuse_blend: a batch needs contiguous [{B},{hw[0]},{hw[1]},{c}] tensors, got {tuple(t.shape)}")
        _lib.check(_L().ff_fuse_blend_images(experts9.data_ptr(), hier3.data_ptr(), guide3.data_ptr(), gates3.data_ptr(), dif1.data_ptr(),
                                             out.data_ptr(), B, Hh, Wh, Hl, Wl, _stream()))
        return out
    _lib.check(_L().ff_fuse_blend(experts9.data_ptr(), hier3.data_ptr(), guide3.data_ptr(), gates3.data_ptr(), dif1.data_ptr(),
                                  out.data_ptr(), Hh, Wh, Hl, Wl, _stream()))
    return out


def tile_accum(tile: T, wy: T, wx: T, acc: T, wsum: T, sy: int, sx: int):
    """acc [1,C,H,W] += tile [1,C,th,tw] * (wy x wx) at (sy, sx); wsum [1,1,H,W] += wy x wx."""
    for t_, n_ in ((tile, "tile"), (wy, "wy"), (wx, "wx"), (acc, "acc"), (wsum, "wsum")):
        _chk(t_, "tile_accum." + n_)
    _, C, th, tw = tile.shape
    _, _, H, W = acc.shape
    _lib.check(_L().ff_tile_accum(tile.contiguous().data_ptr(), C, th, tw, wy.data_ptr(), wx.data_ptr(), acc.data_ptr(),
                                  wsum.data_ptr(), H, W, sy, sx, _stream()))


def tile_normalize(acc: T, wsum: T):
    _, C, H, W = acc.shape
    _lib.check(_L().ff_tile_normalize(acc.data_ptr(), wsum.data_ptr(), C, H, W, _stream()))



D4_CODES = 16


def d4_check_codes(codes, H: int, W: int):
    """Host-side validation of augmentation codes (bit 0 hflip, bit 1 vflip, bits 2-3 k of rot90) for planes of H x W -> list of ints.
    Odd k swaps H and W: a batch must come out with one shape, so it needs square planes."""
    cl = [int(c) for c in codes]
    for c in cl:
        if not 0 <= c < D4_CODES:
            raise _lib.FFError(f"d4 code {c}: expected 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)")
        if (c >> 2) & 1 and H != W:
            raise _lib.FFError(f"d4 code {c} rotates by an odd quarter turn, which needs square planes, got {H}x{W}")
    return cl


def d4_nchw(x: T, codes, out: Optional[T] = None, codes_dev: Optional[T] = None) -> T:
    """The reference's paired augmentation (cached_dataset.py:240-268) of a planar batch [B,C,H,W]: sample b takes the symmetry
    codes[b] = hflip | vflip << 1 | k << 2, applied as flip(-1), flip(-2), rot90(k, (-2, -1)).  `codes` is a host sequence (checked
    here, before any launch); codes_dev, when given, is the same list already on the device (int32 [B]) so that the eight tensors
    of a micro-batch share one upload."""
    _chk(x, "d4_nchw.x")
    if x.dim() != 4 or not x.is_contiguous():
        raise _lib.FFError("d4_nchw: expected a contiguous [B,C,H,W] tensor")
    B, C, H, W = x.shape
    cl = d4_check_codes(codes, H, W)
    if len(cl) != B:
        raise _lib.FFError(f"d4_nchw: {len(cl)} codes for a batch of {B}")
    if codes_dev is None:
        codes_dev = torch.tensor(cl, dtype=torch.int32).to(x.device)
    elif codes_dev.dtype != torch.int32 or not codes_dev.is_cuda or codes_dev.numel() != B or not codes_dev.is_contiguous():
        raise _lib.FFError("d4_nchw: codes_dev must be a contiguous int32 device tensor of B elements")
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk(out, "d4_nchw.out")
        if tuple(out.shape) != tuple(x.shape) or not out.is_contiguous() or out.data_ptr() == x.data_ptr():
            raise _lib.FFError("d4_nchw: out must be a distinct contiguous tensor of x's shape")
    _lib.check(_L().ff_d4_nchw(x.data_ptr(), out.data_ptr(), B, C, H, W, codes_dev.data_ptr(), _stream()))
    return out


# The eight distinct symmetries of the square as d4 codes: k in {0, 1} times the four flip combinations (codes 8..15 repeat them:
# rot90(2) is both flips, rot90(3) is rot90(1) after both flips).
D4_ENSEMBLE = (0, 1, 2, 3, 4, 5, 6, 7)


def d4_inverse_code(code: int) -> int:
    """The d4 code whose transform undoes `code` (both read as flip(-1), flip(-2), rot90(k), in that order).  rot^k after exactly one
    flip is a reflection of the square, hence its own inverse; with none or both flips set (both = a half turn) the transform is a
    rotation, and its inverse keeps the flips and turns back: k' = (4 - k) % 4."""
    c = int(code)
    if not 0 <= c < D4_CODES:
        raise _lib.FFError(f"d4 code {c}: expected 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)")
    if (c & 1) != ((c >> 1) & 1):
        return c
    return (c & 3) | (((4 - (c >> 2)) % 4) << 2)


def d4_canonical_code(code: int) -> int:
    """The code in 0..7 (D4_ENSEMBLE) that names the same symmetry as `code`: a half turn is both flips, so k >= 2 toggles both flip
    bits and keeps k - 2."""
    c = int(code)
    if not 0 <= c < D4_CODES:
        raise _lib.FFError(f"d4 code {c}: expected 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)")
    return c if c < 8 else ((c & 3) ^ 3) | ((c >> 2) - 2) << 2


def d4_rect(x: T, code: int, out: Optional[T] = None, accum: bool = False, scale: float = 1.0) -> T:
    """ONE symmetry (`code` as in d4_nchw: flip(-1), flip(-2), rot90(k, (-2, -1))) of a planar [B,C,H,W] tensor of any H, W: the result
    is [B,C,H,W] for even k and [B,C,W,H] for odd k.  accum=False: out = t * scale; accum=True: out = (out + t) * scale, the add
    rounded before the multiply.  Everything is checked here, before the launch; `out` must not overlap x."""
    _chk(x, "d4_rect.x")
    if x.dim() != 4 or not x.is_contiguous() or x.numel() == 0:
        raise _lib.FFError("d4_rect: expected a non-empty contiguous [B,C,H,W] tensor")
    c = int(code)
    if not 0 <= c < D4_CODES:
        raise _lib.FFError(f"d4 code {c}: expected 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)")
    B, C, H, W = x.shape
    oshape = (B, C, W, H) if (c >> 2) & 1 else (B, C, H, W)
    if out is None:
        if accum:
            raise _lib.FFError("d4_rect: accum=True needs the tensor to accumulate into (out)")
        out = torch.empty(oshape, device=x.device, dtype=torch.float32)
    else:
        _chk(out, "d4_rect.out")
        if tuple(out.shape) != oshape or not out.is_contiguous() or out.device != x.device:
            raise _lib.FFError(f"d4_rect: out must be a contiguous {list(oshape)} tensor on x's device, got {list(out.shape)}")
        nb = 4 * x.numel()
        if out.data_ptr() < x.data_ptr() + nb and x.data_ptr() < out.data_ptr() + nb:
            raise _lib.FFError("d4_rect: out overlaps x (the permutation is not in place)")
    _lib.check(_L().ff_d4_rect_nchw(x.data_ptr(), out.data_ptr(), B, C, H, W, c, 1 if accum else 0, float(scale), _stream()))
    return out


def tile_cut_u8_d4(img_u8: T, code: int, y: int, x: int, th: int, tw: int, out: Optional[T] = None) -> T:
    """The th x tw tile at (y, x) of the TRANSFORMED image d4_rect(u8_to_f32_image(img_u8), code), which is never built: uint8 HWC
    [H,W,3] on the device -> fp32 [1,3,th,tw].  The transformed image is H x W for even k = code >> 2 and W x H for odd k; the tile
    must lie inside it.  Everything is checked here, before the launch."""
    if not (isinstance(img_u8, torch.Tensor) and img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.dim() == 3
            and img_u8.shape[2] == 3 and img_u8.is_contiguous() and img_u8.numel() > 0):
        raise _lib.FFError("tile_cut_u8_d4: expected a non-empty contiguous CUDA(HIP) uint8 [H,W,3] tensor")
    c, y, x, th, tw = int(code), int(y), int(x), int(th), int(tw)
    if not 0 <= c < D4_CODES:
        raise _lib.FFError(f"d4 code {c}: expected 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)")
    H, W, _ = img_u8.shape
    Ht, Wt = (W, H) if (c >> 2) & 1 else (H, W)
    if th < 1 or tw < 1 or y < 0 or x < 0 or y + th > Ht or x + tw > Wt:
        raise _lib.FFError(f"tile_cut_u8_d4: the {th}x{tw} tile at ({y},{x}) leaves the {Ht}x{Wt} transformed image (code {c} of a {H}x{W} image)")
    if out is None:
        out = torch.empty((1, 3, th, tw), device=img_u8.device, dtype=torch.float32)
    else:
        _chk(out, "tile_cut_u8_d4.out")
        if out.numel() != 3 * th * tw or not out.is_contiguous() or out.device != img_u8.device:
            raise _lib.FFError(f"tile_cut_u8_d4: out must be a contiguous float32 tensor of 3x{th}x{tw} elements on the image's device")
    _lib.check(_L().ff_tile_cut_u8_d4(img_u8.data_ptr(), H, W, c, y, x, th, tw, out.data_ptr(), _stream()))
    return out


def tile_fold_d4(acc: T, wsum: T, code: int, ens: Optional[T] = None, accum: bool = False, scale: float = 1.0) -> T:
    """One variant's un-normalised canvas folded into the ensemble accumulator in one pass: with v = acc / max(wsum, 1e-8)
    (tile_normalize's arithmetic) and t = d4_rect(v, code):  accum=False: ens = t * scale;  accum=True: ens = (ens + t) * scale, the
    add rounded before the multiply.  acc [1,3,Hc,Wc] and wsum [1,1,Hc,Wc] are only read; ens is [1,3,Hc,Wc] for even k = code >> 2 and
    [1,3,Wc,Hc] for odd k, and must overlap neither.  Everything is checked here, before the launch."""
    _chk(acc, "tile_fold_d4.acc")
    _chk(wsum, "tile_fold_d4.wsum")
    if acc.dim() != 4 or acc.shape[0] != 1 or acc.shape[1] != 3 or not acc.is_contiguous() or acc.numel() == 0:
        raise _lib.FFError("tile_fold_d4: acc must be a non-empty contiguous [1,3,Hc,Wc] tensor")
    _, _, Hc, Wc = acc.shape
    if wsum.numel() != Hc * Wc or tuple(wsum.shape[-2:]) != (Hc, Wc) or not wsum.is_contiguous() or wsum.device != acc.device:
        raise _lib.FFError(f"tile_fold_d4: wsum must be a contiguous [1,1,{Hc},{Wc}] tensor on acc's device, got {list(wsum.shape)}")
    c = int(code)
    if not 0 <= c < D4_CODES:
        raise _lib.FFError(f"d4 code {c}: expected 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)")
    oshape = (1, 3, Wc, Hc) if (c >> 2) & 1 else (1, 3, Hc, Wc)
    if ens is None:
        if accum:
            raise _lib.FFError("tile_fold_d4: accum=True needs the tensor to accumulate into (ens)")
        ens = torch.empty(oshape, device=acc.device, dtype=torch.float32)
    else:
        _chk(ens, "tile_fold_d4.ens")
        if tuple(ens.shape) != oshape or not ens.is_contiguous() or ens.device != acc.device:
            raise _lib.FFError(f"tile_fold_d4: ens must be a contiguous {list(oshape)} tensor on acc's device, got {list(ens.shape)}")
        e0, e1 = ens.data_ptr(), ens.data_ptr() + 4 * ens.numel()
        for t_, n_ in ((acc, "acc"), (wsum, "wsum")):
            if e0 < t_.data_ptr() + 4 * t_.numel() and t_.data_ptr() < e1:
                raise _lib.FFError(f"tile_fold_d4: ens overlaps {n_} (the fold is not in place)")
    _lib.check(_L().ff_tile_fold_d4(acc.data_ptr(), wsum.data_ptr(), Hc, Wc, c, ens.data_ptr(), 1 if accum else 0, float(scale), _stream()))
    return ens


# ---- cached-expert data-set builder (cache.build_from_folders): patch pairs and the x1/4 degradation ---------------------------------
def crop_pairs_u8(lr_u8: T, hr_u8: T, positions, patch: int) -> Tuple[T, T]:
    """K aligned patch pairs out of one uploaded image pair, one launch: lr_u8 [h,w,3], hr_u8 [4h,4w,3] uint8 HWC on the device,
    positions = host sequence of LR (top, left) -> (lr [K,3,p,p], hr [K,3,4p,4p]) fp32 = u8 / 255, HR patch k at (4 top, 4 left).
    Everything, the positions included, is checked here before the launch."""
    for t, name in ((lr_u8, "lr_u8"), (hr_u8, "hr_u8")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3
                and t.is_contiguous() and t.numel() > 0):
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
    lr = torch.empty((K, 3, p, p), device=lr_u8.device, dtype=torch.float32)
    hr = torch.empty((K, 3, 4 * p, 4 * p), device=lr_u8.device, dtype=torch.float32)
    _lib.check(_L().ff_crop_pairs_u8(lr_u8.data_ptr(), hr_u8.data_ptr(), h, w, pos.data_ptr(), K, p, lr.data_ptr(), hr.data_ptr(), _stream()))
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
    if not (isinstance(pool, torch.Tensor) and pool.is_cuda and pool.dtype == torch.uint8 and pool.dim() == 1 and pool.is_contiguous()
            and pool.numel() > 0):
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
    elif not (desc_dev.is_cuda and desc_dev.dtype == torch.int64 and desc_dev.is_contiguous() and tuple(desc_dev.shape) == (B, 8)
              and desc_dev.device == pool.device):
        raise _lib.FFError(f"sample_pairs_u8: desc_dev must be a contiguous int64 [{B}, 8] tensor on the pool's device")
    shapes = ((B, 3, p, p), (B, 3, 4 * p, 4 * p))
    if out is None:
        lr, hr = (torch.empty(s, device=pool.device, dtype=torch.float32) for s in shapes)
    else:
        lr, hr = out
        for t, s in zip((lr, hr), shapes):
            _chk(t, "sample_pairs_u8.out")
            if tuple(t.shape) != s or not t.is_contiguous() or t.device != pool.device:
                raise _lib.FFError(f"sample_pairs_u8: out must be contiguous {list(shapes[0])} and {list(shapes[1])} tensors on the pool's device")
    _lib.check(_L().ff_sample_pairs_u8(pool.data_ptr(), desc_dev.data_ptr(), B, p, lr.data_ptr(), hr.data_ptr(), _stream()))
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
    for t, name in ((pool, "pool"), (out, "out")):
        _chk(t, "gather_d4_fields." + name)
        if t.dim() != 1 or not t.is_contiguous() or t.numel() < 1:
            raise _lib.FFError(f"gather_d4_fields: {name} must be a non-empty contiguous 1-D fp32 tensor")
    if out.device != pool.device:
        raise _lib.FFError("gather_d4_fields: out must be on the pool's device")
    n = int(n_samples)
    fl = np.ascontiguousarray(np.asarray(fields, dtype=np.int64))
    if fl.ndim != 2 or fl.shape[1] != 5 or not 1 <= fl.shape[0] <= GATHER_MAX_FIELDS or n < 1:
        raise _lib.FFError(f"gather_d4_fields: need 1..{GATHER_MAX_FIELDS} rows of 5 fields and n_samples >= 1, got a table of shape {fl.shape} and {n}")
    if not (isinstance(desc_dev, torch.Tensor) and desc_dev.is_cuda and desc_dev.dtype == torch.int32 and desc_dev.dim() == 2
            and desc_dev.shape[1] == 2 and desc_dev.shape[0] >= 1 and desc_dev.is_contiguous() and desc_dev.device == pool.device):
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
    _lib.check(_L().ff_gather_d4_fields(pool.data_ptr(), n, fl.ctypes.data, int(fl.shape[0]), desc_dev.data_ptr(), B, out.data_ptr(), _stream()))
    _note(0.0, 8.0 * B * float((fl[:, 2] * fl[:, 3] * fl[:, 4]).sum()))
    return [out[oo:oo + B * C * H * W].view(B, C, H, W) for _, oo, C, H, W in fl.tolist()]


def color_jitter_pairs(lr: T, hr: T, table_host, table_dev: Optional[T] = None) -> Tuple[T, T]:
    """The reference's paired colour jitter on a sampled micro-batch, IN PLACE, two launches (csrc/color_jitter.hip): lr [B,3,p,p] and
    hr [B,3,4p,4p] contiguous fp32 device tensors holding u8 / 255 (what sample_pairs_u8 writes); table_host: host fp32 [B][4] rows
    {apply, bf, cf, sf} -- apply 0 leaves the sample's two patches untouched, else brightness bf, contrast cf around each patch's own
    mean, saturation sf through the 8-bit HSV conversion (none when sf == 1).  Every row is checked here before the launch: apply in
    {0, 1}, factors finite and in (0, 2).  table_dev: the same table already on the device (fp32 [B,4]).  -> (lr, hr)."""
    import numpy as np
    for t, name in ((lr, "lr"), (hr, "hr")):
        _chk(t, "color_jitter_pairs." + name)
        if t.dim() != 4 or not t.is_contiguous():
            raise _lib.FFError(f"color_jitter_pairs: {name} must be a contiguous 4-D tensor, got {list(t.shape)}")
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
    elif not (isinstance(table_dev, torch.Tensor) and table_dev.is_cuda and table_dev.dtype == torch.float32 and table_dev.is_contiguous()
              and tuple(table_dev.shape) == (B, 4) and table_dev.device == lr.device):
        raise _lib.FFError(f"color_jitter_pairs: table_dev must be a contiguous float32 [{B}, 4] tensor on lr's device")
    nbytes = int(_L().ff_color_jitter_workspace(B))
    work = torch.empty(nbytes // 8, device=lr.device, dtype=torch.int64)
    _lib.check(_L().ff_color_jitter_pairs(lr.data_ptr(), hr.data_ptr(), table_dev.data_ptr(), B, p, work.data_ptr(), nbytes, _stream()))
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
    _chk(x, "resize_aa.x")
    if x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous() or x.numel() == 0:
        raise _lib.FFError("resize_aa: expected a non-empty contiguous [B,3,H,W] tensor")
    B, C, Hi, Wi = x.shape
    Ho, Wo = (int(v) for v in size)
    if Ho < 1 or Wo < 1 or Hi != 4 * Ho or Wi != 4 * Wo:
        raise _lib.FFError(f"resize_aa: only the x1/4 ratio is built: {Hi}x{Wi} -> {Ho}x{Wo} is refused")
    span_w, wt_w = _aa_tables_dev(Wi, Wo, x.device)
    span_h, wt_h = _aa_tables_dev(Hi, Ho, x.device)
    out = torch.empty((B, C, Ho, Wo), device=x.device, dtype=torch.float32)
    _lib.check(_L().ff_resize_aa(x.data_ptr(), out.data_ptr(), B * C, Hi, Wi, Ho, Wo, span_w.data_ptr(), wt_w.data_ptr(),
                                 span_h.data_ptr(), wt_h.data_ptr(), _stream()))
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
    _chk(x, "resize_cv_cubic.x")
    if x.dim() != 4 or not x.is_contiguous() or x.numel() == 0:
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
        for name, idx, wt, n in (("w", iw, ww, Wo), ("h", ih, wh, Ho)):
            for t, dt in ((idx, torch.int32), (wt, torch.float32)):
                if not torch.is_tensor(t) or t.device != x.device or t.dtype != dt or tuple(t.shape) != (n, 4) or not t.is_contiguous():
                    raise _lib.FFError(f"resize_cv_cubic: the {name} tables must be contiguous int32 / float32 [{n}, 4] tensors on x's device")
    if out is None:
        out = torch.empty((N, C, Ho, Wo), device=x.device, dtype=torch.float32)
    else:
        _chk(out, "resize_cv_cubic.out")
        if tuple(out.shape) != (N, C, Ho, Wo) or not out.is_contiguous() or out.device != x.device:
            raise _lib.FFError(f"resize_cv_cubic: out must be a contiguous [{N},{C},{Ho},{Wo}] tensor on x's device, got {list(out.shape)}")
    _lib.check(_L().ff_resize_cv_cubic(x.data_ptr(), out.data_ptr(), N * C, Hi, Wi, Ho, Wo, tw[0].data_ptr(), tw[1].data_ptr(),
                                       th[0].data_ptr(), th[1].data_ptr(), _stream()))
    _note(0.0, 4.0 * N * C * (Hi * Wi + Ho * Wo))
    return out


for _n in ("conv2d", "cab_fused", "sgfn_tail", "ocab_attn", "ocab_attn_rows16", "token_linear_rows16", "linear", "win_attn_fused", "token_projmlp", "hab_link", "token_linear_gated", "token_mlp", "token_linear", "pixel_mlp", "dwconv3_gate_pool", "naf_front", "naf_ffn", "naf_tail", "window_attn", "layernorm", "pool_mean", "vec_mlp", "dwconv2d", "dwconv3x3_ln", "mix2", "fma3", "affine",
           "nchw_to_nhwc", "nhwc_to_nchw", "resize", "avgpool2", "dct8_bands", "dwt_pass", "fft_bands", "chan_attn_weights", "chan_qkv_attn",
           "band_mha_core", "band_weight", "freq_guidance", "dynamic_gates", "fuse_blend", "tile_accum", "tile_normalize"):
    globals()[_n] = _instrument(globals()[_n])
