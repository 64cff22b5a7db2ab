"""CompleteEnhancedFusionSR (eval mode) on the HIP kernels -- the drop-in for the reference's
`model(lr)` call at models/team29_FreqFusion/io.py:221 (src/models/enhanced_fusion.py:694-754).

    model = FreqFusionHIP(state_dict, device)     # reference-keyed state dict (real or synthetic)
    sr = model(lr)                                # lr [B,3,h,w] fp32 in [0,1] on the GPU -> [B,3,4h,4w]
    sr = model.graphed(lr)                        # same, replayed from a HIP graph cached per input shape
    sr = model.self_ensemble(lr)                  # x8 geometric self-ensemble: the mean over the eight symmetries of the square

There is deliberately no CPU / PyTorch compute path: without a GPU or without libff_hip.so the
constructor raises.
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, Optional

import torch

from . import lib as _lib
from . import ops
from .experts import HatHIP, DatHIP, NafnetHIP
from .fusion import FusionHIP

T = torch.Tensor


def _features_at_lr(raws: list, B: int, h: int, w: int) -> T:
    """Hooked NHWC features (one tensor for the batch, or one per image) -> [B,C,h,w] bilinearly resized to the LR resolution."""
    f = torch.empty((B, raws[0].shape[-1], h, w), device=raws[0].device, dtype=torch.float32)
    n = B // len(raws)
    for i, v in enumerate(raws):
        ops.nhwc_to_nchw(ops.resize(v, (h, w)), out=f[i * n:(i + 1) * n])
    return f


class FreqFusionHIP:
    def __init__(self, state_dict: Dict[str, T], device="cuda:0"):
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.FFError("FreqFusionHIP needs an MI355X (torch device 'cuda'); there is no CPU fallback")
        _lib.load()
        self.dev = dev
        self.multi_stream = os.environ.get("FF_STREAMS", "1") != "0"
        self._side = None
        self._marker = None                              # plan recording: called with "fork" / "join" around the three-stream section
        self._graphs = {}                                # (B,h,w[,lane]) -> (graph, static input, static output)
        self._lanes = None                               # graphed_async: one replay stream per lane
        self.max_graphs = int(os.environ.get("FF_MAX_GRAPHS", "8"))
        with torch.cuda.device(dev):
            self.hat = HatHIP(state_dict, dev)
            self.dat = DatHIP(state_dict, dev)
            self.nafnet = NafnetHIP(state_dict, dev)
            self.fusion = FusionHIP(state_dict, dev)

    @contextlib.contextmanager
    def _fork(self, mark: bool):
        """The three-stream section: the two side streams (made on first use) wait for the caller's stream on entry and the caller's
        stream waits for them on exit.  Yields (side 1, side 2, made); the body appends to `made` every tensor it produces on a side
        stream, and each is handed to the caller's stream (record_stream) after the join.  mark: tell a plan recording where the
        section starts and ends (self._marker)."""
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = (torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev))
        s1, s2 = self._side
        s1.wait_stream(main)
        s2.wait_stream(main)
        if mark and self._marker:
            self._marker("fork")
        made = []
        yield s1, s2, made
        main.wait_stream(s1)
        main.wait_stream(s2)
        if mark and self._marker:
            self._marker("join")
        for t in made:
            t.record_stream(main)

    def _run_experts(self, lr: T, taps: Optional[dict] = None, with_pre: bool = True):
        """ExpertEnsemble.forward_all (expert_loader.py:768-777) for a batch lr [B,3,h,w]: (hat, dat, nafnet [B,3,4h,4w] each, pre or
        None).  The three experts are independent until the fusion stack, so each runs on its own HIP stream (_fork; the
        whole fan-out is captured into the HIP graph): latency-bound kernels of one expert overlap with bandwidth-bound kernels of
        another.  Every expert takes the whole batch through one launch per op (HatHIP / DatHIP / NafnetHIP.forward): HAT on the
        caller's stream, DAT on side stream 1, NAFNet and then (with_pre) the LR-only part of the fusion stack (FusionHIP.pre, once
        for the batch) on side stream 2, the shortest expert's.  On one stream, and
        with taps, the experts run one after the other and pre is left to fusion.forward."""
        if not self.multi_stream or taps is not None:
            hat = self.hat.forward(lr, taps)
            dat = self.dat.forward(lr, taps)
            naf = self.nafnet.forward(lr, taps)
            return hat, dat, naf, None
        with self._fork(mark=True) as (s1, s2, made):
            with torch.cuda.stream(s1):
                dat = self.dat.forward(lr)
            with torch.cuda.stream(s2):
                naf = self.nafnet.forward(lr)
                pre = self.fusion.pre(lr) if with_pre else None
            hat = self.hat.forward(lr)
            made += (dat, naf, *self.fusion.pre_tensors(pre))
        return hat, dat, naf, pre

    def experts(self, lr: T, taps: Optional[dict] = None, with_pre: bool = False):
        """The experts of ONE image lr [1,3,h,w]: {hat, dat, nafnet: [1,3,4h,4w]}, or with with_pre ({...}, pre), pre being
        FusionHIP.pre(lr) on three streams and None otherwise."""
        hat, dat, naf, pre = self._run_experts(lr, taps, with_pre)
        ex = {"hat": hat, "dat": dat, "nafnet": naf}
        return (ex, pre) if with_pre else ex

    @torch.no_grad()
    def experts_with_features(self, lr: T, streams: bool = False):
        """ExpertEnsemble.forward_all_with_hooks (expert_loader.py:894-951): ({hat,dat,nafnet} SR outputs [B,3,4h,4w],
        {hat [B,180,h,w], dat [B,180,h,w], nafnet [B,64,h,w]} hook features bilinearly resized to the LR resolution, NCHW).
        The payload of the cached-expert files (isr2_amd/cache.py).  streams=True runs the same launches with DAT and NAFNet (and
        their feature resizes) on the two side streams of forward(), forked from and joined to the caller's stream: the same bits,
        the small grids of one expert beside those of another (cache.build_from_folders).
        All three experts run the batch through one launch per op.  Every image's tensors are those of its own B == 1 call, bit
        for bit."""
        if lr.dim() != 4 or lr.shape[0] < 1 or lr.shape[1] != 3:
            raise _lib.FFError(f"expected lr of shape [B,3,h,w], got {tuple(lr.shape)}")
        lr = lr.to(self.dev, torch.float32).contiguous()
        B, _, h, w = lr.shape
        nets = {"hat": self.hat, "dat": self.dat, "nafnet": self.nafnet}

        def fwd(name):                                         # -> (SR output [B,3,4h,4w], [hooked NHWC features])
            raw = {}
            return nets[name].forward(lr, feats=raw), [raw[name]]

        with torch.cuda.device(self.dev):
            if streams:
                outs, feats = {}, {}
                with self._fork(mark=False) as (s1, s2, made):
                    for name, s in (("dat", s1), ("nafnet", s2), ("hat", torch.cuda.current_stream())):
                        with torch.cuda.stream(s):
                            outs[name], raws = fwd(name)
                            feats[name] = _features_at_lr(raws, B, h, w)
                    made += (outs["dat"], outs["nafnet"], feats["dat"], feats["nafnet"])
            else:
                done = {name: fwd(name) for name in nets}          # the three forwards, then the three feature resizes
                outs = {name: o for name, (o, _) in done.items()}
                feats = {name: _features_at_lr(raws, B, h, w) for name, (_, raws) in done.items()}
        return {k: outs[k] for k in nets}, {k: feats[k] for k in nets}

    @torch.no_grad()
    def forward_with_precomputed(self, lr: T, expert_outputs, expert_features=None, taps: Optional[dict] = None) -> T:
        """CompleteEnhancedFusionSR.forward_with_precomputed (enhanced_fusion.py:756-812): the cached-mode forward.  The expert
        outputs {hat,dat,nafnet: [B,3,4h,4w]} and, optionally, their hooked features [B,C,h,w] (isr2_amd/cache.py files, or
        experts_with_features()) come from the caller; only the fusion stack runs (one launch per op for the batch, FusionHIP.forward),
        with the collaborative block live when features are given.  A [3,..] / [C,..] tensor is one image.  taps: B == 1 only.
        The forward half of SURVEY 8f rank 1; no backward is built."""
        if lr.dim() != 4 or lr.shape[0] < 1 or lr.shape[1] != 3:
            raise _lib.FFError(f"expected lr of shape [B,3,h,w], got {tuple(lr.shape)}")
        lr = lr.to(self.dev, torch.float32).contiguous()
        B, _, h, w = lr.shape
        if B > 1 and taps is not None:
            raise _lib.FFError("taps are recorded for B == 1 only")
        ex = {}
        for k in ("hat", "dat", "nafnet"):
            t = expert_outputs[k]
            t = t.unsqueeze(0) if t.dim() == 3 else t
            if tuple(t.shape) != (B, 3, 4 * h, 4 * w):
                raise _lib.FFError(f"expert output {k}: expected [{B},3,{4 * h},{4 * w}], got {tuple(t.shape)}")
            ex[k] = t.to(self.dev, torch.float32).contiguous()
        feats = None
        if expert_features is not None:
            feats = {k: (v.unsqueeze(0) if v.dim() == 3 else v).to(self.dev, torch.float32).contiguous() for k, v in expert_features.items()}
            for k, v in feats.items():
                if v.dim() != 4 or v.shape[0] != B:
                    raise _lib.FFError(f"expert feature {k}: expected [{B},C,h,w], got {tuple(v.shape)}")
        with torch.cuda.device(self.dev):
            return self.fusion.forward(lr, ex, taps, feats=feats)

    @torch.no_grad()
    def forward(self, lr: T, taps: Optional[dict] = None, out: Optional[T] = None) -> T:
        if lr.dim() != 4 or lr.shape[0] < 1 or lr.shape[1] != 3:
            raise _lib.FFError(f"expected lr of shape [B,3,h,w], got {tuple(lr.shape)}")
        lr = lr.to(self.dev, torch.float32).contiguous()
        B, _, h, w = lr.shape
        # Every global op of the path is per image (average pools, channel attention statistics, rFFT2, squeeze gates), so a batch is
        # B independent images.  The three experts take the whole batch through one launch per op (HatHIP / DatHIP / NafnetHIP.forward:
        # their per-image quantities -- HAT's channel-attention gate [B,180], DAT's attention matrix [B,180,180] and channel gate [B,180],
        # NAFNet's SCA vector [B,c] -- are matrices) and so does the fusion stack (FusionHIP.pre / .forward: the rFFT2 band planes, the
        # gates and the zero-padded concat buffers are [B,...]; the collaborative gains of the cached mode [B,3]).  No image is copied:
        # the kernels that read the planar LR batch take an image at any 4-byte offset, so a batch of any size can be recorded as a plan.
        # Bit-identical to B single forwards: every image is computed in the kernel forms of its own B == 1 forward.
        if B > 1 and taps is not None:
            raise _lib.FFError("taps are recorded for B == 1 only")
        if out is None:
            out = torch.empty((B, 3, 4 * h, 4 * w), device=self.dev, dtype=torch.float32)
        with torch.cuda.device(self.dev):
            hat, dat, naf, pre = self._run_experts(lr, taps)
            if taps is not None:
                taps.update({"expert.hat": hat, "expert.dat": dat, "expert.nafnet": naf})
            self.fusion.forward(lr, {"hat": hat, "dat": dat, "nafnet": naf}, taps, pre=pre, out=out)
        return out

    __call__ = forward

    @torch.no_grad()
    def graphed(self, lr: T) -> T:
        """forward(lr) replayed from a HIP graph cached per input shape (captured on the first call with that shape: one
        warm-up on a side stream, then the capture).  The whole launch sequence -- ~1400 kernels on three streams -- becomes
        one hipGraphLaunch; tiles of one shape (io._tiled_forward, bench.py) replay the same graph.  The returned tensor is
        the graph's static output buffer: consume it (or clone it) before the next graphed() call of the same shape."""
        graph, static_in, static_out = self._graph_for(lr, 0)
        static_in.copy_(lr, non_blocking=True)               # device-to-device memcpy into the captured input buffer
        graph.replay()
        return static_out

    def _graph_for(self, lr: T, lane: int):
        lr = lr.to(self.dev, torch.float32)
        key = tuple(lr.shape) + ((lane,) if lane else ())
        ent = self._graphs.get(key)
        if ent is None:
            if len(self._graphs) >= self.max_graphs:          # each graph pins its own activation pool: keep a few shapes only
                torch.cuda.synchronize(self.dev)              # (a replay of the evicted graph may still be in flight on a lane)
                old = next(iter(self._graphs))
                self._graphs.pop(old)
                ops.drop_persistent(key=(id(self),) + old)   # the concat / padded-input buffers that graph's launches point at
            ops.set_lane(lane)
            ops.set_capture_key((id(self),) + key)
            try:
                with torch.cuda.device(self.dev):
                    static_in = lr.clone().contiguous()
                    cur = torch.cuda.current_stream()
                    side = torch.cuda.Stream(device=self.dev)
                    side.wait_stream(cur)
                    with torch.cuda.stream(side):
                        self.forward(static_in)
                    cur.wait_stream(side)
                    torch.cuda.synchronize(self.dev)
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        static_out = self.forward(static_in)
            finally:
                ops.set_lane(0)
                ops.set_capture_key(None)
            ent = self._graphs[key] = (graph, static_in, static_out)
        return ent

    def graphed_async(self, lr: T, lane: int):
        """Two-deep tile pipeline: like graphed(), but the replay runs on the lane's own stream (lane 0 / 1, each with its own
        captured graph, static buffers and persistent scratch), so the tail of one tile -- the fusion stack's small grids after the
        three experts have joined -- overlaps the head of the next.  Returns (static output, event): wait for the event on the
        consuming stream before reading the output; work the caller has queued on the current stream (the previous consumer of
        this lane's output included) is ordered before the replay.  Tiles of one image are independent (io._tiled_forward)."""
        if lane not in (0, 1):
            raise _lib.FFError("graphed_async: lane must be 0 or 1")
        graph, static_in, static_out = self._graph_for(lr, lane + 1)  # own graph + persistent scratch per lane (0 is the synchronous path's); first use captures on the CURRENT stream
        if self._lanes is None:
            self._lanes = (torch.cuda.Stream(device=self.dev), torch.cuda.Stream(device=self.dev))
        ls = self._lanes[lane]
        ls.wait_stream(torch.cuda.current_stream())
        src = lr.to(self.dev, torch.float32)
        src.record_stream(ls)                                 # the caller may drop the tile before the lane has copied it
        with torch.cuda.stream(ls):
            static_in.copy_(src, non_blocking=True)
            graph.replay()
            ev = torch.cuda.Event()
            ev.record(ls)
        return static_out, ev

    @torch.no_grad()
    def self_ensemble(self, lr: T, run=None, run_async=None, codes=ops.D4_ENSEMBLE, out: Optional[T] = None) -> T:
        """Geometric self-ensemble (the "x8" / forward_x8 test-time pass of HAT's and EDSR's test code): the model runs on the
        symmetries `codes` of lr [B,3,h,w], every output is mapped back and the results are averaged.  Pinned bit for bit:

            acc = inv_0(run(T_0(lr)))
            acc = acc + inv_i(run(T_i(lr)))     i = 1 .. n-1 in the order of `codes`, fp32, one rounding per add
            out = acc * (1 / n)                 fused into the last accumulation (n = 8: an exact power-of-two scale)

        with T_i = ops.d4_rect(., codes[i]) and inv_i = ops.d4_rect(., ops.d4_inverse_code(codes[i]), out=acc, accum=i > 0, ...)
        (csrc/augment.hip: ff_d4_rect_nchw): two permutation launches per variant around the forward, no other glue.  A variant with
        an odd quarter turn is [B,3,w,h]; its output comes back as [B,3,4h,4w].

        run(x) -> [B,3,4H,4W] defaults to self.forward.  A run that returns a static graph buffer (self.graphed) is safe: the
        accumulate launch that reads the buffer is stream-ordered before the next replay that overwrites it.  run_async(x, lane)
        -> (output, event) (self.graphed_async) is used when every variant has lr's shape (h == w): the variants alternate over the
        two lanes exactly as the tiles of io._tiled_forward do, and their outputs are consumed in code order on the current stream,
        so the result is bit-identical to the sequential loop.  A non-square lr ignores run_async.

        Empty codes, a code outside 0..15 and two codes that name the same symmetry raise FFError before any launch."""
        if not isinstance(lr, torch.Tensor) or lr.dim() != 4 or lr.shape[0] < 1 or lr.shape[1] != 3 or lr.shape[2] < 1 or lr.shape[3] < 1:
            raise _lib.FFError(f"self_ensemble: expected lr of shape [B,3,h,w], got {tuple(getattr(lr, 'shape', ()))}")
        cl = [int(c) for c in codes]
        if not cl:
            raise _lib.FFError("self_ensemble: no symmetry codes given")
        inv = [ops.d4_inverse_code(c) for c in cl]                       # raises on a code outside 0..15
        canon = [ops.d4_canonical_code(c) for c in cl]
        if len(set(canon)) != len(cl):
            raise _lib.FFError(f"self_ensemble: codes {cl} name a symmetry twice (codes 8..15 repeat 0..7)")
        B, _, h, w = lr.shape
        oshape = (B, 3, 4 * h, 4 * w)
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != oshape or out.dtype != torch.float32
                                or out.device != self.dev or not out.is_contiguous()):
            raise _lib.FFError(f"self_ensemble: out must be a contiguous float32 {list(oshape)} tensor on {self.dev}")
        lr = lr.to(self.dev, torch.float32).contiguous()
        if run is None:
            run = self.forward
        if h != w:
            run_async = None
        n = len(cl)
        with torch.cuda.device(self.dev):
            acc = out if out is not None else torch.empty(oshape, device=self.dev, dtype=torch.float32)

            def fold(sr, i):                                   # d4_rect refuses an sr whose mapped-back shape is not acc's
                ops.d4_rect(sr.contiguous(), inv[i], out=acc, accum=i > 0, scale=1.0 / n if i == n - 1 else 1.0)

            if run_async is None:
                for i, c in enumerate(cl):
                    fold(run(ops.d4_rect(lr, c)), i)
                return acc
            pend = [None, None]

            def consume(lane):
                if pend[lane] is not None:
                    sr, ev, i = pend[lane]
                    torch.cuda.current_stream().wait_event(ev)
                    fold(sr, i)
                    pend[lane] = None

            for i, c in enumerate(cl):
                lane = i & 1
                consume(lane)                                  # variant i-2: its output buffer is about to be overwritten
                sr, ev = run_async(ops.d4_rect(lr, c), lane)
                pend[lane] = (sr, ev, i)
            consume(n & 1)
            consume((n + 1) & 1)
            return acc
