"""The whole-image path's kernels on operands whose element offsets pass 2^30 / 2^31 / 2^32 (run with -m gpu on the MI355X).

One case per launch of tests/golden/bigextent_calls.json (op, kernel route, contraction mode, operand pitches and channels): the launches of
one whole-image forward of BASELINE config 4 (2040x1356 LR, 5424x8160 HR) that touch an operand of rows * ld >= 2^30 elements.

Shape.  The real row width (HR 8160, or the width the launch had), the launch's pitches and channel counts, and the smallest height that
still crosses the boundary T: H = P * (ceil(T / (P * W * ld)) + 2) with ld the smallest pitch among the operands the table marks at or past
T, so every marked operand crosses T and the last two periods lie wholly past it; no operand is larger than the table's (plan() below:
P = 32, or 16 / 48 / 24 where 32 does not fit or would make T a whole number of periods).  T = 2^31 for a
launch with an operand marked ge31 (and a second case at 2^32 where one is marked ge32); T = 2^30 for the launches whose largest operand
is in [2^30, 2^31) -- 2^30 floats are 2^32 bytes, the boundary of a 32-bit BYTE offset.

Construction.  Every input is vertically periodic: a slab of P rows of seeded normals (rnd of tests/test_ops_gpu.py) tiled k times by a
broadcast copy.  Checks, over the whole output: (value) the same op on a 3-period slab against PyTorch fp32 at the bar
tests/test_ops_gpu.py / tests/test_naf_tail_gpu.py holds that op to in that mode; (position independence) periods 1 .. k-2 of the big
output are bit-equal to the slab call's middle period, periods 0 and k-1 (which see the image border) to its first and last -- so the
value bar holds for every element of the big output; (nothing else touched) an output that is a channel slice of a wider buffer leaves
every other column at the sentinel; (reductions) a pooled mean from the same launch against the fp64 sums of the expected periods;
(route) the kernel route is the table's.  The slab call is forced onto the big call's route where ops would pick another one for a small
input (the LDS-resident 3x3 kernel takes inputs below 2^31 elements only: the slab call runs with set_halo(False) when the big call is an
implicit GEMM).  The implicit GEMMs choose their tile form from the row count M only through M >= 16384 (bf16) / 65536 (f32) -- a
3-period slab is 783 360 rows -- so both calls take the same form; ff_conv2d_bf16s_tile is asserted to agree.
"""
import json
import math
import os
import time

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
T30, T31, T32 = 2 ** 30, 2 ** 31, 2 ** 32
SENT = 7.25                                  # sentinel of the columns a launch must not touch
PR = 32                                      # period in output rows (16 where needed): a multiple of the tile heights (8, 16) and of the 4-row strips
GEOM = {5424 * 8160: 8160, 5440 * 8192: 8192, 2712 * 4080: 4080, 2720 * 4096: 4096, 1356 * 2040: 2040, 1360 * 2048: 2048}   # rows -> image width
ROWS_W = 8160                                # row-wise ops (no spatial neighbourhood): periods of PR * 8160 rows, a multiple of 256

GEMM_TOL = {"f32": 2e-5, "bf16x3": 6e-5, "bf16": 2e-2}      # tests/test_ops_gpu.py
BF16_TOL = 1.5e-2                                            # tests/test_ops_gpu.py, plain-bf16 forms of the fused token kernels
BF16_FFN_TOL = 3e-2                                          # tests/test_ops_gpu.py / tests/test_naf_tail_gpu.py: naf_front, naf_ffn, naf_tail
ACTF = {None: lambda t: t, "gelu": F.gelu, "relu": F.relu, "sigmoid": torch.sigmoid, "lrelu": lambda t: F.leaky_relu(t, 0.01)}

# launches of the table this module does not pin: none.  (A launch a regenerated table adds must be given a family here, be an entry that
# refuses its extent (REFUSED), or be named in UNPINNED_OPS with a reason from UNPINNED_REASONS: tests/test_bigextent_cpu.py holds the closure.)
UNPINNED_REASONS = {}
UNPINNED_OPS = {}
REFUSED = []                                 # entries that reject their recorded extent: none, the forward ran every launch of the table


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import lib
    lib.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    return torch.device("cuda:0")


def rnd(*shape, dev, seed=0, scale=1.0):
    from test_ops_gpu import rnd as _rnd
    return _rnd(*shape, dev=dev, seed=seed, scale=scale)


_SLABS = {}


def slab(shape, dev, seed, scale=1.0, shift=0.0, dtype=torch.float32):
    """A seeded slab, made once per (shape, seed) and shared by the cases (never written)."""
    key = (tuple(shape), seed, scale, shift, dtype)
    if key not in _SLABS:
        if sum(v.numel() * v.element_size() for v in _SLABS.values()) > 4 * 2 ** 30:
            _SLABS.clear()
        _SLABS[key] = (rnd(*shape, dev=dev, seed=seed, scale=scale) + shift).to(dtype)
    return _SLABS[key]


class Buf:
    """[k * P, W, C] operand at channel offset `off` of a [k * P, W, ld] buffer.  Input: the slab tiled k times, the other columns at SENT.
    Output (slab None): everything at SENT."""

    def __init__(self, k, P, W, C, ld, dev, src=None, dtype=torch.float32):
        self.k, self.P, self.W, self.C, self.ld = k, P, W, C, ld
        self.off = 4 if ld - C >= 4 else 0
        self.buf = torch.empty((k * P, W, ld), device=dev, dtype=dtype)
        if src is None or ld != C:
            self.buf.fill_(SENT)
        if src is not None:
            assert tuple(src.shape) == (P, W, C)
            self.buf.view(k, P, W, ld)[..., self.off:self.off + C] = src
        self.t = self.buf[..., self.off:self.off + C]

    @property
    def nhwc(self):
        return self.t.unsqueeze(0)

    @property
    def rows(self):
        return self.buf.view(-1, self.ld)[:, self.off:self.off + self.C]

    @property
    def nchw(self):
        return self.t.permute(2, 0, 1).unsqueeze(0).float()

    def untouched(self):
        o, C = self.off, self.C
        return bool((self.buf[..., :o] == SENT).all()) and bool((self.buf[..., o + C:] == SENT).all())


def hwc(t_nchw):
    return t_nchw[0].permute(1, 2, 0)


# ---- the launch families ----------------------------------------------------------------------------------------------------------------
# A family object describes one launch of the table: operand geometry (role -> (P, W, C, ld) per period), make(k) -> inputs,
# call(inp) -> {name: [k * P, W, C] output}, ref(inp3) -> the same names from PyTorch fp32, tol(name), and optional pool handling.
class Family:
    border = False                           # True: periods 0 and k - 1 see the image border

    def __init__(self, d, dev):
        self.d, self.dev, self.mode = d, dev, d["mode"]
        self.a, self.small, self.o = d["args"], set(d["small"]), d["operands"]
        self.P = PR                          # period in output rows; the test halves it when PR-row periods would outgrow the recorded operand

    def ld(self, role):
        return self.o[role][1]

    def ch(self, role):
        return self.o[role][2]

    def has(self, role):
        return role in self.o or role in self.small

    def vec(self, n, seed, scale=1.0, shift=0.0):
        return (rnd(n, dev=self.dev, seed=seed, scale=scale) + shift).contiguous()

    def inbuf(self, k, role, P, W, seed, scale=1.0, shift=0.0):
        dt = torch.bfloat16 if self.o[role][0] == "bfloat16" else torch.float32
        return Buf(k, P, W, self.ch(role), self.ld(role), self.dev, slab((P, W, self.ch(role)), self.dev, seed, scale, shift, dt), dt)

    def outbuf(self, k, role, P, W):
        return Buf(k, P, W, self.ch(role), self.ld(role), self.dev)

    def out_role(self):
        return "out" if "out" in self.o else "ret0"

    def route_ok(self, inp):
        return True


def rows_geom(fam):
    return {r: (fam.P, ROWS_W) for r in fam.o if r != "w"}


class Linear(Family):
    def geom(self):
        return rows_geom(self)

    def __init__(self, d, dev):
        super().__init__(d, dev)
        N, K = self.o["w"][1:]
        self.N, self.K = N, K
        self.w = rnd(N, K, dev=dev, seed=11, scale=1.0 / math.sqrt(K))
        self.b = self.vec(N, 12, 0.1) if "bias" in self.small else None
        self.mul = self.vec(N, 13) if "mul" in self.small else None
        self.kmul = self.vec(K, 14, 0.5, 1.0) if "kmul" in self.small else None
        self.alpha = 0.7 if "alpha" in self.a else 1.0

    def make(self, k):
        inp = {"x": self.inbuf(k, "x", self.P, ROWS_W, 1)}
        if "res" in self.o:
            inp["res"] = self.inbuf(k, "res", self.P, ROWS_W, 2)
        if "out" in self.o:
            inp["out"] = self.outbuf(k, "out", self.P, ROWS_W)
        return inp

    def call(self, inp):
        from isr2_amd import ops
        out = ops.linear(inp["x"].rows, self.w, self.b, act=self.a.get("act"), res=inp["res"].rows if "res" in inp else None, mul=self.mul,
                         alpha=self.alpha, out=inp["out"].rows if "out" in inp else None, kmul=self.kmul, dynamic_w=bool(self.a.get("dynamic_w")))
        return {"y": out.unflatten(0, (-1, ROWS_W))}

    def ref(self, inp):
        x = inp["x"].t.float()
        y = ACTF[self.a.get("act")](F.linear(x * self.kmul if self.kmul is not None else x, self.w, self.b))
        if self.mul is not None:
            y = y * self.mul
        y = y * self.alpha
        return {"y": y + inp["res"].t if "res" in inp else y}

    def tol(self, name):
        return GEMM_TOL[self.mode]

    def route_ok(self, inp):
        from isr2_amd import ops
        kinds = [k for k, _ in ops.PREPARED.of(self.w)]
        want = {"igemm_f32": [], "igemm_bf16s": [] if self.a.get("dynamic_w") else ["split"], "rows_gemm": ["split"]}[self.d["route"]]
        bf16_in = inp["x"].buf.dtype == torch.bfloat16
        return kinds == want and bf16_in == (self.d["route"] == "rows_gemm")


class Conv2d(Family):
    def __init__(self, d, dev):
        super().__init__(d, dev)
        self.kh, self.kw = self.a["ksize"]
        self.st, self.pad, self.sh = self.a["stride"][0], tuple(self.a["pad"]), self.a.get("shuffle", 0)
        self.Cout, K = self.o["w"][1:]
        self.Cin = K // (self.kh * self.kw)
        self.w4 = rnd(self.Cout, self.Cin, self.kh, self.kw, dev=dev, seed=21, scale=1.0 / math.sqrt(K))
        from isr2_amd.prep import pack_conv
        self.wp = pack_conv(self.w4)
        self.b = self.vec(self.Cout, 22, 0.1) if "bias" in self.small else None
        self.mul = self.vec(self.Cout, 23) if "mul" in self.small else None
        self.alpha = 0.7 if "alpha" in self.a else 1.0
        self.border = self.kh > 1 and self.st == 1
        self.Win = GEOM[self.o["x"][3]]
        self.Wout = self.Win // self.st * (2 if self.sh else 1)

    @property
    def Pin(self):
        return self.P * self.st // (2 if self.sh else 1)

    def geom(self):
        g = {"x": (self.Pin, self.Win), self.out_role(): (self.P, self.Wout)}
        if "res" in self.o:
            g["res"] = (self.P, self.Wout)
        return g

    def make(self, k):
        inp = {"x": self.inbuf(k, "x", self.Pin, self.Win, 3)}
        if "res" in self.o:
            inp["res"] = self.inbuf(k, "res", self.P, self.Wout, 4)
        if "out" in self.o:
            inp["out"] = self.outbuf(k, "out", self.P, self.Wout)
        return inp

    def call(self, inp):
        from isr2_amd import ops, lib
        hint, halo, x = 0, ops._HALO, inp["x"]
        if self.d["route"] == "igemm_bf16s":
            vec4 = 1 if (x.ld % 4 == 0 and self.Cin % 4 == 0) else 0
            K = self.kh * self.kw * self.Cin
            Mo = x.k * self.P * self.Wout // (4 if self.sh else 1)
            hint = int(lib.load().ff_conv2d_bf16s_tile(Mo, self.Cout, K, vec4))
            assert hint == int(lib.load().ff_conv2d_bf16s_tile(T31 - 1, self.Cout, K, vec4))      # the form does not depend on M here
            if x.k == 3:
                ops.set_halo(False)                  # a slab is small enough for the LDS-resident kernel; the big input is not
        try:
            out = ops.conv2d(inp["x"].nhwc, self.wp, self.b, ksize=(self.kh, self.kw), stride=(self.st, self.st), pad=self.pad, act=self.a.get("act"),
                             res=inp["res"].nhwc if "res" in inp else None, mul=self.mul, alpha=self.alpha, shuffle=self.sh,
                             out=inp["out"].nhwc if "out" in inp else None, tile_hint=hint, per_image=True)
        finally:
            ops.set_halo(halo)
        return {"y": out[0]}

    def ref(self, inp):
        y = ACTF[self.a.get("act")](F.conv2d(inp["x"].nchw, self.w4, self.b, stride=self.st, padding=self.pad))
        if self.mul is not None:
            y = y * self.mul.view(1, -1, 1, 1)
        y = y * self.alpha
        if self.sh:
            y = F.pixel_shuffle(y, 2)
        y = hwc(y)
        return {"y": y + inp["res"].t if "res" in inp else y}

    def tol(self, name):
        return 3e-6 if self.d["route"] == "conv3x3_small" else GEMM_TOL[self.mode]       # test_conv3x3_small_matches_torch's bar

    def route_ok(self, inp):
        from isr2_amd import ops
        kinds = sorted(k for k, _ in ops.PREPARED.of(self.wp))
        want = {"igemm_f32": [], "igemm_bf16s": ["split"], "conv3x3_small": ["small"], "halo": ["halo" if self.mode == "bf16x3" else "halo1"]}
        x = inp["x"]
        if self.d["route"] == "igemm_bf16s" and self.kh == 3 and self.st == 1 and self.Cin >= 32 and self.Cin % 4 == 0 and x.ld % 4 == 0 \
                and x.k > 3 and self.Cout <= 64:
            assert x.buf.numel() >= T31              # the only reason this launch is not the LDS-resident kernel's: its input extent
        return kinds == want[self.d["route"]]


class TokenLinear(Family):
    def geom(self):
        return rows_geom(self)

    def __init__(self, d, dev):
        super().__init__(d, dev)
        pk = self.a["pk"]
        self.N, self.K = pk["N"], pk["K"]
        from isr2_amd.prep import pack_token_linear
        self.w = rnd(self.N, self.K, dev=dev, seed=31, scale=1.0 / math.sqrt(self.K))
        self.b = self.vec(self.N, 32, 0.1)
        self.pk = pack_token_linear(self.w, self.b)
        self.g = self.vec(self.K, 33, 0.1, 1.0) if "gamma" in self.small else None
        self.be = self.vec(self.K, 34, 0.1) if "beta" in self.small else None

    def make(self, k):
        inp = {"x": self.inbuf(k, "x", self.P, ROWS_W, 5, 1.5, 0.3)}
        if "res" in self.o:
            inp["res"] = self.inbuf(k, "res", self.P, ROWS_W, 6)
        return inp

    def call(self, inp):
        from isr2_amd import ops
        sr = tuple(self.a["stats_range"]) if "stats_range" in self.a else None
        out = ops.token_linear(inp["x"].rows, self.pk, gamma=self.g, beta=self.be, act=self.a.get("act"), res=inp["res"].rows if "res" in inp else None,
                               stats_range=sr)
        if sr is not None:
            return {"y": out[0].unflatten(0, (-1, ROWS_W)), "stats": out[1].unflatten(0, (-1, ROWS_W))}
        return {"y": out.unflatten(0, (-1, ROWS_W))}

    def ref(self, inp):
        x = inp["x"].t
        if self.g is not None:
            x = F.layer_norm(x, (self.K,), self.g, self.be, 1e-5)
        y = ACTF[self.a.get("act")](F.linear(x, self.w, self.b))
        return {"y": y + inp["res"].t if "res" in inp else y}          # (the stats side output: position independence only)

    def tol(self, name):
        return 6e-5 if self.mode == "bf16x3" else BF16_TOL


class NafFront(Family):
    border = True

    def __init__(self, d, dev):
        super().__init__(d, dev)
        C = self.C = self.ch("x")
        from isr2_amd.prep import pack_token_linear, pack_dw
        self.g, self.be = self.vec(C, 41, 0.1, 1.0), self.vec(C, 42, 0.1)
        self.w1, self.b1 = rnd(2 * C, C, dev=dev, seed=43, scale=1.0 / math.sqrt(C)), self.vec(2 * C, 44, 0.1)
        self.w2, self.b2 = rnd(2 * C, 1, 3, 3, dev=dev, seed=45, scale=0.3), self.vec(2 * C, 46, 0.1)
        self.pk, self.wt = pack_token_linear(self.w1, self.b1), pack_dw(self.w2)
        self.W = GEOM[self.o["x"][3]]

    def geom(self):
        return {"x": (self.P, self.W), "ret0": (self.P, self.W)}

    def make(self, k):
        return {"x": self.inbuf(k, "x", self.P, self.W, 7, 1.5, 0.2)}

    def call(self, inp):
        from isr2_amd import ops
        out, pooled = ops.naf_front(inp["x"].nhwc, self.pk, self.g, self.be, self.wt, self.b2)
        return {"y": out[0], "pool": pooled[0]}

    def ref(self, inp):
        x, C = inp["x"].nchw, self.C
        mu = x.mean(1, keepdim=True)
        var = (x - mu).pow(2).mean(1, keepdim=True)
        xn = (x - mu) / (var + 1e-6).sqrt() * self.g.view(1, -1, 1, 1) + self.be.view(1, -1, 1, 1)
        t = F.conv2d(F.conv2d(xn, self.w1.view(2 * C, C, 1, 1), self.b1), self.w2, self.b2, padding=1, groups=2 * C)
        return {"y": hwc(t[:, :C] * t[:, C:])}

    def tol(self, name):
        return 2 * GEMM_TOL["bf16x3"] if self.mode == "bf16x3" else BF16_FFN_TOL


class NafFfn(Family):
    def geom(self):
        return rows_geom(self)

    def __init__(self, d, dev):
        super().__init__(d, dev)
        C = self.C = self.a["pk"]["C"]
        s = 1.0 / math.sqrt(C)
        self.kw = dict(w3=rnd(C, C, dev=dev, seed=51, scale=s), b3=self.vec(C, 52, 0.1), w4=rnd(2 * C, C, dev=dev, seed=53, scale=s),
                       b4=self.vec(2 * C, 54, 0.1), w5=rnd(C, C, dev=dev, seed=55, scale=s), b5=self.vec(C, 56, 0.1),
                       sca=self.vec(C, 57, 0.3, 1.0), beta=self.vec(C, 58, 0.4), gamma=self.vec(C, 59, 0.3), ln_g=self.vec(C, 60, 0.1, 1.0),
                       ln_b=self.vec(C, 61, 0.1))
        from isr2_amd.prep import pack_naf_ffn, pack_naf_tail
        k = self.kw
        self.tail = d["op"] == "naf_tail"
        self.pk = pack_naf_tail(k["w3"], k["b3"], k["w4"], k["b4"], k["w5"], k["b5"]) if self.tail else pack_naf_ffn(k["w4"], k["b4"], k["w5"], k["b5"])

    def make(self, k):
        if self.tail:
            return {"g": self.inbuf(k, "g", self.P, ROWS_W, 8), "x": self.inbuf(k, "x", self.P, ROWS_W, 9, 1.3, 0.2)}
        return {"y": self.inbuf(k, "y", self.P, ROWS_W, 9, 1.3, 0.2)}

    def call(self, inp):
        from isr2_amd import ops
        k = self.kw
        if self.tail:
            out = ops.naf_tail(inp["g"].rows, inp["x"].rows, self.pk, k["sca"], k["beta"], k["ln_g"], k["ln_b"], k["gamma"])
        else:
            out = ops.naf_ffn(inp["y"].rows, self.pk, k["ln_g"], k["ln_b"], k["gamma"])
        return {"y": out.unflatten(0, (-1, ROWS_W))}

    def ref(self, inp):
        k, C = self.kw, self.C
        y = inp["x"].t + k["beta"] * F.linear(inp["g"].t * k["sca"], k["w3"], k["b3"]) if self.tail else inp["y"].t
        h = F.linear(F.layer_norm(y, (C,), k["ln_g"], k["ln_b"], 1e-6), k["w4"], k["b4"])
        return {"y": y + k["gamma"] * F.linear(h[..., :C] * h[..., C:], k["w5"], k["b5"])}

    def tol(self, name):
        return 6e-5 if self.mode == "bf16x3" else BF16_FFN_TOL


class Mix2(Family):
    def geom(self):
        return rows_geom(self)

    def make(self, k):
        inp = {"a": self.inbuf(k, "a", self.P, ROWS_W, 71)}
        for r, s in (("b", 72), ("pa", 73)):
            if r in self.o:
                inp[r] = self.inbuf(k, r, self.P, ROWS_W, s)
        if "out" in self.o:
            inp["out"] = self.outbuf(k, "out", self.P, ROWS_W)
        return inp

    def call(self, inp):
        from isr2_amd import ops
        self.ka, self.kb = (0.7 if "ka" in self.a else 1.0), (0.3 if "kb" in self.a else 1.0)
        out = ops.mix2(inp["a"].rows, inp["b"].rows if "b" in inp else None, ka=self.ka, kb=self.kb, pa=inp["pa"].rows if "pa" in inp else None,
                       out=inp["out"].rows if "out" in inp else None)
        return {"y": out.unflatten(0, (-1, ROWS_W))}

    def ref(self, inp):
        y = self.ka * inp["a"].t
        if "pa" in inp:
            y = y * inp["pa"].t
        return {"y": y + self.kb * inp["b"].t if "b" in inp else y}

    def tol(self, name):
        return 1e-6


class Fma3(Family):
    def geom(self):
        return rows_geom(self)

    def make(self, k):
        return {r: self.inbuf(k, r, self.P, ROWS_W, 80 + i) for i, r in enumerate(("a", "b", "c")) if r in self.o}

    def call(self, inp):
        from isr2_amd import ops
        self.alpha = 0.1 if "alpha" in self.a else 1.0
        return {"y": ops.fma3(inp["a"].rows if "a" in inp else None, inp["b"].rows, inp["c"].rows, self.alpha).unflatten(0, (-1, ROWS_W))}

    def ref(self, inp):
        y = self.alpha * inp["b"].t * inp["c"].t
        return {"y": inp["a"].t + y if "a" in inp else y}

    def tol(self, name):
        return 1e-6


class Affine(Family):
    def geom(self):
        return rows_geom(self)

    def make(self, k):
        self.sc, self.sf = self.vec(self.ch("x"), 91), self.vec(self.ch("x"), 92)
        return {"x": self.inbuf(k, "x", self.P, ROWS_W, 90)}

    def call(self, inp):
        from isr2_amd import ops
        return {"y": ops.affine(inp["x"].rows, self.sc, self.sf, self.a.get("act")).unflatten(0, (-1, ROWS_W))}

    def ref(self, inp):
        return {"y": ACTF[self.a.get("act")](inp["x"].t * self.sc + self.sf)}

    def tol(self, name):
        return 1e-6


class LayerNorm(Family):
    def geom(self):
        return rows_geom(self)

    def make(self, k):
        C = self.ch("x")
        self.g, self.be = self.vec(C, 101, 0.1, 1.0), self.vec(C, 102, 0.1)
        return {"x": self.inbuf(k, "x", self.P, ROWS_W, 100, 2.0, 0.5)}

    def call(self, inp):
        from isr2_amd import ops
        return {"y": ops.layernorm(inp["x"].rows, self.g, self.be).unflatten(0, (-1, ROWS_W))}

    def ref(self, inp):
        return {"y": F.layer_norm(inp["x"].t, (self.ch("x"),), self.g, self.be, 1e-5)}

    def tol(self, name):
        return 1e-5


class PixelMlp(Family):
    def geom(self):
        return rows_geom(self)

    def make(self, k):
        C = self.ch("x")
        self.W1, self.b1, self.w2 = rnd(8, C, dev=self.dev, seed=111, scale=1.0 / math.sqrt(C)), self.vec(8, 112, 0.1), rnd(1, 8, dev=self.dev, seed=113, scale=0.5)
        return {"x": self.inbuf(k, "x", self.P, ROWS_W, 110)}

    def call(self, inp):
        from isr2_amd import ops
        return {"y": ops.pixel_mlp(inp["x"].rows, self.W1, self.b1, self.a["act1"], self.w2, 0.37, self.a["act2"]).unflatten(0, (-1, ROWS_W))}

    def ref(self, inp):
        return {"y": ACTF[self.a["act2"]](F.linear(ACTF[self.a["act1"]](F.linear(inp["x"].t, self.W1, self.b1)), self.w2) + 0.37)}

    def tol(self, name):
        return 1e-5


class BandMha(Family):
    PP = 32 * 1020                           # pixels per period; a period is PP * nbands rows

    def geom(self):
        return {r: (self.PP * self.a["nbands"] // ROWS_W, ROWS_W) for r in ("qkv", "ret0")}

    def make(self, k):
        return {"qkv": self.inbuf(k, "qkv", self.PP * self.a["nbands"] // ROWS_W, ROWS_W, 120)}

    def call(self, inp):
        from isr2_amd import ops
        q = inp["qkv"]
        return {"y": ops.band_mha_core(q.rows, q.k * self.PP, self.a["nbands"], self.a["heads"]).unflatten(0, (-1, ROWS_W))}

    def ref(self, inp):
        nb, heads = self.a["nbands"], self.a["heads"]
        qkv = inp["qkv"].rows
        E = qkv.shape[-1] // 3
        q, k, v = [t.reshape(-1, nb, heads, 16).transpose(1, 2) for t in qkv.chunk(3, dim=-1)]
        ref = (torch.softmax((q * 0.25) @ k.transpose(-2, -1), dim=-1) @ v).transpose(1, 2).reshape(-1, E)
        return {"y": ref.unflatten(0, (-1, ROWS_W))}

    def tol(self, name):
        return 1e-5


class Resize(Family):
    border = True

    def __init__(self, d, dev):
        super().__init__(d, dev)
        self.Wi, self.Wo = GEOM[self.o["x"][3]], self.a["size"][1]
        self.s = self.Wo // self.Wi
        assert self.Wo == self.s * self.Wi and self.a["mode"] == "bilinear"
        self.mul = 0.8 if "mul" in self.a else 1.0

    def geom(self):
        return {"x": (self.P // self.s, self.Wi), "out": (self.P, self.Wo)}

    def make(self, k):
        return {"x": self.inbuf(k, "x", self.P // self.s, self.Wi, 130), "out": self.outbuf(k, "out", self.P, self.Wo)}

    def call(self, inp):
        from isr2_amd import ops
        o = inp["out"]
        ops.resize(inp["x"].nhwc, (o.k * self.P, self.Wo), out=o.nhwc, mul=self.mul)
        return {"y": o.t}

    def ref(self, inp):
        x = inp["x"]
        return {"y": hwc(F.interpolate(x.nchw, size=(self.s * x.k * x.P, self.Wo), mode="bilinear", align_corners=False)) * self.mul}

    def tol(self, name):
        return 2e-6

    def route_ok(self, inp):                 # ff_resize's own test for the four-channel kernel
        x, o = inp["x"], inp["out"]
        v4 = x.C % 4 == 0 and x.ld % 4 == 0 and o.ld % 4 == 0 and x.t.data_ptr() % 16 == 0 and o.t.data_ptr() % 16 == 0
        return v4 == self.d["route"].startswith("vec4")


class DwGatePool(Family):
    border = True

    def __init__(self, d, dev):
        super().__init__(d, dev)
        C2 = self.ch("t")
        from isr2_amd.prep import pack_dw
        self.w, self.b = rnd(C2, 1, 3, 3, dev=dev, seed=141, scale=0.3), self.vec(C2, 142, 0.1)
        self.wt = pack_dw(self.w)
        self.W = GEOM[self.o["t"][3]]

    def geom(self):
        return {"t": (self.P, self.W), "ret0": (self.P, self.W)}

    def make(self, k):
        return {"t": self.inbuf(k, "t", self.P, self.W, 140)}

    def call(self, inp):
        from isr2_amd import ops
        g, pooled = ops.dwconv3_gate_pool(inp["t"].nhwc, self.wt, self.b)
        return {"y": g[0], "pool": pooled[0]}

    def ref(self, inp):
        C = self.ch("t") // 2
        dd = F.conv2d(inp["t"].nchw, self.w, self.b, padding=1, groups=2 * C)
        return {"y": hwc(dd[:, :C] * dd[:, C:])}

    def tol(self, name):
        return 1e-5


class DwConv2d(Family):
    border = True

    def __init__(self, d, dev):
        super().__init__(d, dev)
        C = self.C = self.ch("x")
        self.kh, self.kw = self.a["ksize"]
        from isr2_amd.prep import pack_dw
        self.w = rnd(C, 1, self.kh, self.kw, dev=dev, seed=151, scale=0.3)
        self.wt = pack_dw(self.w)
        self.b = self.vec(C, 152, 0.1) if "bias" in self.small else None
        self.ps = self.vec(C, 153, 0.1, 1.0) if "post_scale" in self.small else None
        self.pt = self.vec(C, 154, 0.1) if "post_shift" in self.small else None
        self.W = GEOM[self.o["x"][3]]

    def geom(self):
        return {r: (self.P, self.W) for r in self.o}

    def make(self, k):
        inp = {"x": self.inbuf(k, "x", self.P, self.W, 150)}
        if "mul_in" in self.o:
            inp["mul_in"] = self.inbuf(k, "mul_in", self.P, self.W, 155)
        return inp

    def call(self, inp):
        from isr2_amd import ops
        out = ops.dwconv2d(inp["x"].nhwc, self.wt, self.b, ksize=(self.kh, self.kw), pad=tuple(self.a["pad"]), post_scale=self.ps, post_shift=self.pt,
                           act=self.a.get("act"), mul_in=inp["mul_in"].nhwc if "mul_in" in inp else None)
        return {"y": out[0]}

    def ref(self, inp):
        y = F.conv2d(inp["x"].nchw, self.w, self.b, padding=tuple(self.a["pad"]), groups=self.C)
        if self.ps is not None:
            y = y * self.ps.view(1, -1, 1, 1) + self.pt.view(1, -1, 1, 1)
        y = hwc(ACTF[self.a.get("act")](y))
        return {"y": y * inp["mul_in"].t if "mul_in" in inp else y}

    def tol(self, name):
        return 1e-5


class DwConvLn(Family):
    border = True

    def __init__(self, d, dev):
        super().__init__(d, dev)
        C = self.C = self.ch("x")
        from isr2_amd.prep import pack_dw
        self.w, self.b = rnd(C, 1, 3, 3, dev=dev, seed=161, scale=0.3), self.vec(C, 162, 0.1)
        self.wt = pack_dw(self.w)
        self.g, self.be = self.vec(C, 163, 0.1, 1.0), self.vec(C, 164, 0.1)
        self.W = GEOM[self.o["x"][3]]

    def geom(self):
        return {r: (self.P, self.W) for r in self.o}

    def make(self, k):
        x = self.inbuf(k, "x", self.P, self.W, 160, 1.5, 0.3)
        xs = x.t[:self.P]
        st = torch.stack((xs.mean(-1), 1.0 / torch.sqrt(xs.var(-1, unbiased=False) + 1e-5)), dim=-1).contiguous()
        return {"x": x, "mul_in": self.inbuf(k, "mul_in", self.P, self.W, 165), "stats": Buf(k, self.P, self.W, 2, 2, self.dev, st)}

    def call(self, inp):
        from isr2_amd import ops
        return {"y": ops.dwconv3x3_ln(inp["x"].nhwc, self.wt, self.b, inp["stats"].rows, self.g, self.be, mul_in=inp["mul_in"].nhwc)[0]}

    def ref(self, inp):
        xn = F.layer_norm(inp["x"].t, (self.C,), self.g, self.be, 1e-5).permute(2, 0, 1).unsqueeze(0)
        return {"y": hwc(F.conv2d(xn, self.w, self.b, padding=1, groups=self.C)) * inp["mul_in"].t}

    def tol(self, name):
        return 1e-4                          # test_sgfn_layernorm_on_load's bar for this kernel


class SgfnTail(Family):
    border = True

    def __init__(self, d, dev):
        super().__init__(d, dev)
        c2 = self.c2 = self.a["c2"]
        N = self.N = self.ch("ret0")
        from isr2_amd.prep import pack_dw
        self.wd, self.bd = rnd(c2, 1, 3, 3, dev=dev, seed=171, scale=0.3), self.vec(c2, 172, 0.1)
        self.wt = pack_dw(self.wd)
        self.g, self.be = self.vec(c2, 173, 0.1, 1.0), self.vec(c2, 174, 0.1)
        self.w2, self.b2 = rnd(N, c2, dev=dev, seed=175, scale=1.0 / math.sqrt(c2)), self.vec(N, 176, 0.1)
        self.W = GEOM[self.o["y"][3]]

    def geom(self):
        return {r: (self.P, self.W) for r in self.o if r != "w2"}

    def make(self, k):
        y = self.inbuf(k, "y", self.P, self.W, 170)
        x2 = y.t[:self.P, :, self.c2:2 * self.c2]
        st = torch.stack((x2.mean(-1), 1.0 / torch.sqrt(x2.var(-1, unbiased=False) + 1e-5)), dim=-1).contiguous()
        return {"y": y, "res": self.inbuf(k, "res", self.P, self.W, 177), "stats": Buf(k, self.P, self.W, 2, 2, self.dev, st)}

    def call(self, inp):
        from isr2_amd import ops
        return {"y": ops.sgfn_tail(inp["y"].nhwc, self.c2, self.wt, self.bd, inp["stats"].rows, self.g, self.be, self.w2, self.b2, res=inp["res"].nhwc)[0]}

    def ref(self, inp):
        c2 = self.c2
        yd = inp["y"].t.double()
        x2n = F.layer_norm(yd[..., c2:2 * c2], (c2,), self.g.double(), self.be.double(), 1e-5).permute(2, 0, 1).unsqueeze(0)
        gate = yd[..., :c2] * hwc(F.conv2d(x2n, self.wd.double(), self.bd.double(), padding=1, groups=c2))
        return {"y": (inp["res"].t.double() + F.linear(gate, self.w2.double(), self.b2.double())).float()}

    def tol(self, name):
        return GEMM_TOL["bf16"]              # test_sgfn_tail_fused's bar


class WindowAttn(Family):
    """Window attention on a [k * 32, 2048] token grid: 32 rows are whole windows of every shape in the table (16x16, 8x32, 32x8), so the grid
    of (shifted) windows repeats with the period; Hp = H here (the recorded DAT launches pad 1360 rows to 1376: the padded bottom windows are
    the border period's business and are covered at small sizes by tests/test_ops_gpu.py)."""
    border = True

    def __init__(self, d, dev):
        super().__init__(d, dev)
        a = self.a
        self.heads, self.dd = a["heads"], a["d"]
        self.win, self.kwin, self.shift = tuple(a["win"]), tuple(a["kwin"]), tuple(a["shift"])
        self.q_off, self.k_off, self.v_off, self.o_off = a.get("q_off", 0), a["k_off"], a["v_off"], a.get("o_off", 0)
        self.W = a["W"]
        assert GEOM[self.o["qkv"][3]] == self.W
        wh, ww = self.win
        if self.kwin != self.win:            # HAT OCAB: the reference's wrapped table indices
            from test_ops_gpu import _hat_bias
            table = rnd((wh + self.kwin[0] - 1) ** 2, self.heads, dev=dev, seed=181, scale=0.5)
            self.bias = _hat_bias(table, wh, self.kwin[0], self.heads)
        else:                                # one value per relative offset (HAT's table, DAT's DynamicPosBias output)
            rel = rnd(self.heads, (2 * wh - 1) * (2 * ww - 1), dev=dev, seed=182, scale=0.5)
            cy, cx = torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="ij")
            cy, cx = cy.reshape(-1).to(dev), cx.reshape(-1).to(dev)
            idx = (cy[:, None] - cy[None, :] + wh - 1) * (2 * ww - 1) + (cx[:, None] - cx[None, :] + ww - 1)
            self.bias = rel[:, idx].contiguous()
        self.biasT = self.bias.transpose(1, 2).contiguous()

    def geom(self):
        return {"qkv": (self.P, self.W), "out": (self.P, self.W)}

    def make(self, k):
        return {"qkv": self.inbuf(k, "qkv", self.P, self.W, 180), "out": self.outbuf(k, "out", self.P, self.W)}

    def call(self, inp):
        from isr2_amd import ops
        q, o = inp["qkv"], inp["out"]
        H = q.k * self.P
        ops.window_attn(q.nhwc, o.nhwc, self.biasT, q_off=self.q_off, k_off=self.k_off, v_off=self.v_off, o_off=self.o_off, H=H, W=self.W, Hp=H,
                        Wp=self.W, win=self.win, kwin=self.kwin, shift=self.shift, use_mask=bool(self.a.get("use_mask")), heads=self.heads,
                        d=self.dd, scale=self.dd ** -0.5)
        return {"y": o.t[..., self.o_off:self.o_off + self.heads * self.dd]}

    def ref(self, inp):
        from oracle import freqfusion_oracle as O
        qkv = inp["qkv"].nhwc
        H, W, hd, heads, d = qkv.shape[1], self.W, self.heads * self.dd, self.heads, self.dd
        (wh, ww), (kh, kw), (sh, sw) = self.win, self.kwin, self.shift
        q, kk, v = [qkv[..., o:o + hd] for o in (self.q_off, self.k_off, self.v_off)]
        if self.kwin != self.win:
            nwin = (H // wh) * (W // ww)
            kv = torch.cat((kk, v), -1).permute(0, 3, 1, 2)
            kvw = F.unfold(kv, kernel_size=kh, stride=wh, padding=(kh - wh) // 2)
            kvw = kvw.reshape(1, 2, hd, kh * kw, nwin).permute(1, 0, 4, 3, 2).reshape(2, nwin, kh * kw, hd)
            qh = O._win_split(q, wh, ww).reshape(-1, wh * ww, heads, d).transpose(1, 2) * d ** -0.5
            kh_ = kvw[0].reshape(-1, kh * kw, heads, d).transpose(1, 2)
            vh = kvw[1].reshape(-1, kh * kw, heads, d).transpose(1, 2)
            o = O._softmax_attn(qh, kh_, vh, self.bias, None).transpose(1, 2).reshape(-1, wh * ww, hd)
            return {"y": O._win_merge(o, wh, ww, H, W)[0]}
        t = [q, kk, v]
        if sh or sw:
            t = [torch.roll(u, shifts=(-sh, -sw), dims=(1, 2)) for u in t]
        tw = [O._win_split(u, wh, ww).reshape(-1, wh * ww, heads, d).transpose(1, 2) for u in t]
        mask = O._region_mask(H, W, wh, ww, sh, sw).to(self.dev) if self.a.get("use_mask") else None
        o = O._softmax_attn(tw[0] * d ** -0.5, tw[1], tw[2], self.bias, mask).transpose(1, 2).reshape(-1, wh * ww, hd)
        o = O._win_merge(o, wh, ww, H, W)
        if sh or sw:
            o = torch.roll(o, shifts=(sh, sw), dims=(1, 2))
        return {"y": o[0]}

    def tol(self, name):
        return GEMM_TOL[self.mode]           # test_window_attn_hat / _ocab / _dat_branches


def _ocab_perm(dev, heads=6, d=30):
    """Column 32 t + j of the head-padded rows <- channel (heads d) (t // heads) + d (t % heads) + j of the fp32 q | k | v rows; pads -> -1."""
    p = torch.full((3 * heads * 32,), -1, dtype=torch.long)
    for t in range(3 * heads):
        p[32 * t:32 * t + d] = heads * d * (t // heads) + d * (t % heads) + torch.arange(d)
    return p.to(dev)


class TokenLinearRows16(Family):
    def geom(self):
        return rows_geom(self)

    def __init__(self, d, dev):
        super().__init__(d, dev)
        pk = self.a["pk"]
        self.K, self.heads, self.dd = pk["K"], pk["heads"], pk["d"]
        C = self.heads * self.dd
        from isr2_amd.prep import pack_ocab_qkv
        self.w, self.b = rnd(3 * C, self.K, dev=dev, seed=191, scale=self.K ** -0.5), self.vec(3 * C, 192)
        self.pk = pack_ocab_qkv(self.w, self.b, self.heads, self.dd)
        self.g, self.be = self.vec(self.K, 193, 0.1, 1.0), self.vec(self.K, 194, 0.1)

    def make(self, k):
        return {"x": self.inbuf(k, "x", self.P, ROWS_W, 190)}

    def call(self, inp):
        from isr2_amd import ops
        out = ops.token_linear_rows16(inp["x"].rows, self.pk, gamma=self.g, beta=self.be)
        assert out.dtype == torch.bfloat16 and out.stride(0) == self.ld("ret0")
        return {"y": out.unflatten(0, (-1, ROWS_W))}

    def ref(self, inp):
        perm = _ocab_perm(self.dev, self.heads, self.dd)
        real = perm >= 0
        y32 = F.linear(F.layer_norm(inp["x"].t, (self.K,), self.g, self.be, 1e-5), self.w, self.b)
        ref = torch.zeros(tuple(y32.shape[:-1]) + (perm.numel(),), device=self.dev)          # the pad columns are exact zeros
        ref[..., real] = y32[..., perm[real]] * self.pk["scale"][real]
        return {"y": ref}

    def tol(self, name):
        return BF16_TOL


class OcabRows16(Family):
    border = True

    def __init__(self, d, dev):
        super().__init__(d, dev)
        a = self.a
        self.heads, self.dd, self.ws, self.ows, self.W = a["heads"], a["d"], a["ws"], a["ows"], a["W"]
        assert GEOM[self.o["qkv16"][3]] == self.W
        from test_ops_gpu import _hat_bias
        from isr2_amd.prep import pack_rel_overlap
        table = rnd((self.ws + self.ows - 1) ** 2, self.heads, dev=dev, seed=201, scale=0.5)
        self.bias, self.rel = _hat_bias(table, self.ws, self.ows, self.heads), pack_rel_overlap(table, self.ws, self.ows)

    def geom(self):
        return {"qkv16": (self.P, self.W), "out": (self.P, self.W)}

    def make(self, k):
        C = self.heads * self.dd
        q32 = slab((self.P, self.W, 3 * C), self.dev, 200)
        perm = _ocab_perm(self.dev, self.heads, self.dd)
        real = perm >= 0
        sc = torch.ones(perm.numel(), device=self.dev)
        sc[:self.heads * 32] = float(torch.tensor(self.dd ** -0.5, dtype=torch.float32))
        rows = torch.zeros((self.P, self.W, perm.numel()), device=self.dev, dtype=torch.bfloat16)
        rows[..., real] = (q32[..., perm[real]] * sc[real]).bfloat16()                        # bf16(q * scale), bf16(k), bf16(v): what the kernel reads
        o = Buf(k, self.P, self.W, self.ch("out"), self.ld("out"), self.dev, dtype=torch.bfloat16)
        return {"qkv16": Buf(k, self.P, self.W, perm.numel(), self.ld("qkv16"), self.dev, rows, torch.bfloat16), "out": o, "q32": q32}

    def call(self, inp):
        from isr2_amd import ops
        q, o = inp["qkv16"], inp["out"]
        ops.ocab_attn_rows16(q.nhwc, o.nhwc, self.rel, q_off=0, k_off=self.a["k_off"], v_off=self.a["v_off"], H=q.k * self.P, W=self.W,
                             heads=self.heads, d=self.dd, ws=self.ws, ows=self.ows)
        return {"y": o.t}

    def ref(self, inp):
        from oracle import freqfusion_oracle as O
        heads, d, ws, ows, W = self.heads, self.dd, self.ws, self.ows, self.W
        C = heads * d
        qkv = inp["q32"].repeat(3, 1, 1).unsqueeze(0)
        H = qkv.shape[1]
        q = O._win_split(qkv[..., :C], ws, ws)
        kv = qkv[..., C:].permute(0, 3, 1, 2)
        nwin = (H // ws) * (W // ws)
        kvw = F.unfold(kv, kernel_size=ows, stride=ws, padding=(ows - ws) // 2)
        kvw = kvw.reshape(1, 2, C, ows * ows, nwin).permute(1, 0, 4, 3, 2).reshape(2, nwin, ows * ows, C)
        qh = q.reshape(-1, ws * ws, heads, d).transpose(1, 2) * d ** -0.5
        kh = kvw[0].reshape(-1, ows * ows, heads, d).transpose(1, 2)
        vh = kvw[1].reshape(-1, ows * ows, heads, d).transpose(1, 2)
        o = O._softmax_attn(qh, kh, vh, self.bias, None).transpose(1, 2).reshape(-1, ws * ws, C)
        return {"y": O._win_merge(o, ws, ws, H, W)[0]}

    def tol(self, name):
        return GEMM_TOL["bf16"]              # test_ocab_attn_persistent's bar


class ChanAttn(Family):
    """DAT's channel attention weights: a [180, 180] reduction over every token, so there is no output period to compare.  The input is made
    position DEPENDENT instead: q is periodic, k is the periodic slab with its sign flipped in the last two periods (the ones wholly past T).
    The gram is then (k - 4) / k times one period's and both norms are sqrt(k) times one period's: softmax(temp * (k - 4) / k * cos) is the
    expected block, from one period in fp64.  A launch that read those periods from the low rows, or not at all, gives another factor."""
    reduction = True

    def geom(self):
        return {"qkv": (self.P, ROWS_W)}

    def make(self, k):
        self.temp = self.vec(6, 211, 0.2, 1.0)
        b = self.inbuf(k, "qkv", self.P, ROWS_W, 210)
        q = b.t[:self.P, :, :180]
        mix = rnd(180, 180, dev=self.dev, seed=212, scale=180 ** -0.5)
        kk = (q @ mix + 0.5 * b.t[:self.P, :, 180:360]).contiguous()                           # k correlated with q: cosines of O(0.1 .. 1)
        v = b.buf.view(k, self.P, ROWS_W, b.ld)
        v[..., b.off + 180:b.off + 360] = kk
        v[k - 2:, ..., b.off + 180:b.off + 360] *= -1.0
        return {"qkv": b}

    def call(self, inp):
        from isr2_amd import ops
        return {"w": ops.chan_attn_weights(inp["qkv"].rows, 0, self.a["k_off"], self.temp)}

    def ref(self, inp):
        b = inp["qkv"]
        k, heads, d = b.k, 6, 30
        q = b.t[:self.P, :, :180].reshape(-1, heads, d).permute(1, 2, 0).double()
        kk = b.t[:self.P, :, 180:360].reshape(-1, heads, d).permute(1, 2, 0).double()
        cos = F.normalize(q, dim=-1) @ F.normalize(kk, dim=-1).transpose(-2, -1)
        a = torch.softmax(cos * ((k - 4) / k) * self.temp.double()[:, None, None], dim=-1)
        return {"w": torch.block_diag(*[a[h] for h in range(heads)]).float()}

    def tol(self, name):
        return 1e-5                          # test_chan_attn_weights' bar


FAMILIES = {"linear": Linear, "conv2d": Conv2d, "token_linear": TokenLinear, "naf_front": NafFront, "naf_ffn": NafFfn, "naf_tail": NafFfn,
            "mix2": Mix2, "fma3": Fma3, "affine": Affine, "layernorm": LayerNorm, "pixel_mlp": PixelMlp, "band_mha_core": BandMha,
            "resize": Resize, "dwconv3_gate_pool": DwGatePool, "dwconv2d": DwConv2d, "dwconv3x3_ln": DwConvLn, "sgfn_tail": SgfnTail,
            "window_attn": WindowAttn, "token_linear_rows16": TokenLinearRows16, "ocab_attn_rows16": OcabRows16, "chan_attn_weights": ChanAttn}


def builder_of(d):
    return FAMILIES.get(d["op"])


def refused(d):
    return d["op"] in REFUSED


def unpinned(d):
    return UNPINNED_OPS.get(d["op"])


class Case:
    def __init__(self, launch, T):
        self.launch, self.T = launch, T
        o = {r: v for r, v in launch["operands"].items() if r != "w"}
        big = max(o, key=lambda r: o[r][1] * o[r][3])
        self.id = "-".join([launch["op"], launch["route"], launch["mode"], f"{big}{o[big][1]}c{o[big][2]}",
                            "w" + "x".join(str(v) for v in launch["operands"]["w"][1:]) if "w" in launch["operands"] else
                            "".join(f"{k[0]}{v}" for k, v in sorted(launch["args"].items()) if not isinstance(v, dict))[:24],
                            {T30: "2p30", T31: "2p31", T32: "2p32"}[T]]).replace(" ", "").replace("[", "").replace("]", "").replace(",", "x").replace("!=", "ne")


def _cases():
    with open(os.path.join(HERE, "golden", "bigextent_calls.json")) as f:
        table = json.load(f)
    out, seen = [], {}
    for call in table["launches"]:
        d = json.loads(call)
        if builder_of(d) is None:
            continue
        ext = [v[1] * v[3] for r, v in d["operands"].items() if r != "w"]
        levels = [T31] if max(ext) >= T31 else [T30]
        if max(ext) >= T32:
            levels.append(T32)
        for T in levels:
            c = Case(d, T)
            n = seen[c.id] = seen.get(c.id, 0) + 1
            if n > 1:
                c.id += f"-{n}"
            out.append(c)
    return out


CASES = _cases()


def periods(t, k):
    return t.unflatten(0, (k, t.shape[0] // k))


def check_periods(big, small, k, name):
    """big [k * P, ...] against the 3-period slab call: first, middle (all of them) and last period, bit for bit."""
    b, s = periods(big, k), periods(small, 3)
    assert b.shape[1:] == s.shape[1:], name
    assert torch.equal(b[0], s[0]), f"{name}: period 0 differs from the slab call's first period"
    assert torch.equal(b[k - 1], s[2]), f"{name}: period {k - 1} differs from the slab call's last period"
    same = (b[1:k - 1] == s[1]).flatten(1).all(dim=1)
    bad = (~same).nonzero().flatten().tolist()
    assert not bad, f"{name}: periods {[i + 1 for i in bad[:8]]} (of {k}) differ from the slab call's middle period"


def plan(fam, d, T):
    """The period (fam.P) and the number of periods k of a case: the smallest height that puts two whole periods of every operand the table
    marks at or past T beyond T, with no operand larger than the forward's own.  32-row periods; 16 where 32 would outgrow the recorded
    operand; 48 / 24 where the width is a power of two (HAT / DAT pad the HR grid to 8192): there a 32-row period of a 64-pitch operand is
    2^24 elements, T would be a whole number of periods, and an offset wrapped by T would land on the SAME phase and read the same values."""
    o = {r: v for r, v in d["operands"].items() if r != "w"}
    marked = [r for r in o if o[r][1] * o[r][3] >= T]
    for fam.P in (PR, PR // 2, 48, 24):
        geom = fam.geom()
        assert marked and all(r in geom for r in marked), (marked, sorted(geom))
        per = {r: geom[r][0] * geom[r][1] for r in geom}                 # rows per period
        k = max(-(-T // (per[r] * o[r][1])) for r in marked) + 2
        if all(k * per[r] <= o[r][3] for r in geom) and all(T % (per[r] * o[r][1]) for r in marked):
            break
    for r in geom:
        assert k * per[r] <= o[r][3], (r, k * per[r], o[r][3])          # stays inside the sizes the forward produces
        if r in marked:
            assert (k - 2) * per[r] * o[r][1] >= T                       # the last two periods lie wholly past T
            assert T % (per[r] * o[r][1]), "an offset wrapped by T must land on another phase of the period"
    return k


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_launch_past_the_boundary(dev, case):
    from isr2_amd import ops
    from test_ops_gpu import close
    d, T = case.launch, case.T
    t0, k = time.perf_counter(), 0
    torch.cuda.reset_peak_memory_stats()
    prev = ops.gemm_mode()
    ops.set_gemm_mode(d["mode"])
    try:
        fam = FAMILIES[d["op"]](d, dev)
        k = plan(fam, d, T)
        inp = fam.make(k)
        big = fam.call(inp)
        torch.cuda.synchronize()
        assert fam.route_ok(inp), f"route is not the table's {d['route']}"
        for r, b in inp.items():
            if r == "out":
                assert b.untouched(), "columns outside the output slice were written"
        if getattr(fam, "reduction", False):                             # no output period: the expected block of the big call itself
            for name, exp in fam.ref(inp).items():
                close(big[name], exp, fam.tol(name), f"{case.id} {name}")
            print(f"[bigextent] {case.id}: k = {k}, {time.perf_counter() - t0:.2f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
            return
        inp3 = fam.make(3)
        small = fam.call(inp3)
        ref = fam.ref(inp3)
        for name, exp in ref.items():
            close(small[name], exp, fam.tol(name), f"{case.id} {name} (slab)")
            check_periods(big[name], small[name], k, name)
        if "stats" in big:
            check_periods(big["stats"], small["stats"], k, "stats")
        if "pool" in big:                                                # the launch's own mean over the whole extent
            e = periods(ref["y"].double(), 3).flatten(1, 2).sum(1)       # [3, C] fp64 sums of the expected periods
            n = ref["y"].shape[0] // 3 * ref["y"].shape[1]
            want = ((e[0] + (k - 2) * e[1] + e[2]) / (k * n)).float()
            close(big["pool"], want, fam.tol("pool"), f"{case.id} pooled mean")
        if "out" in inp3:
            assert inp3["out"].untouched()
    except RuntimeError as e:                                            # a device fault ends the session: nothing more is launched after it
        if any(w in str(e) for w in ("HIP error", "hipError", "illegal memory access", "hardware exception")):
            pytest.exit(f"GPU fault in {case.id}: {e}", returncode=3)
        raise
    finally:
        ops.set_gemm_mode(prev)
        inp = inp3 = big = small = ref = fam = None                       # (the prepared weight images die with their weights)
        torch.cuda.empty_cache()
    print(f"[bigextent] {case.id}: k = {k}, {time.perf_counter() - t0:.2f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
