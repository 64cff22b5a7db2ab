"""CPU checks of tests/golden/train_ref.py, the fp64 references tests/test_train_kernels_gpu.py holds the training kernels to.
No GPU: a stand-in plays each kernel's arithmetic in fp32 -- the same fp32 products, summed STRICTLY SEQUENTIALLY in pixel order
(np.add.accumulate in float32), the worst of the orders the kernels use -- over the case tables of train_ref (the GPU test imports
the same tables).

  * the stand-in passes every per-element assertion of the module;
  * the constants of the reductions are re-measured: the worst |stand-in - ref| / (2^-24 mag) per family stays within
    *_MEASURED * 1.25, and the module's constants equal 4 * *_MEASURED;
  * fp64 torch.autograd of the plain torch formula agrees with every reference to 1e-12 * mag: the references are the right operations;
  * every mutant of a stand-in FAILS the assertion in every case it applies to.  A mutant the assertion cannot tell from the stand-in is
    reported by name and fails the test unless UNDETECTABLE lists it with its reason.

BatchNorm (training mode), the bilinear adjoint, the two DFT passes and the AdamW + EMA step have stand-ins and autograd / torch.optim
checks but no mutants (none is asked of them); the loss and squared-norm sums are held to the DERIVED
train_ref.c_flat_sum against a stand-in that plays the kernels' own order, because a sequential sum of 262147 positive terms is no
model of a tree.

Mutants (family: name):
    wgrad: last_col (x < W - 1), tail8 (columns beyond the last multiple of 8 dropped), last_chunk (the rows of the last chunk
           dropped), swap_kykx, pad (padding off by one), prev_image (a tap above an image's first row reads the previous image's last
           row), no_acc (accumulate ignored), chan (the last channel of a partial co / ci tile taken from its neighbour)
    reduce: last_row (of every group), shift (group boundary one row late), y_col (y per row read with the column index), scale2
    unary: every inclusive comparison made strict and every strict one inclusive, sgn(0) = 1, the softplus threshold inclusive,
           sigmoid_bwd fed x instead of y, notail (sigmoid and softplus_bwd as 1 / (1 + exp(-x)) throughout: exp(100) overflows and
           sigmoid(-100) = 3.8e-44 comes back 0, which is what the kernel did before this reference existed)
    layernorm_bwd: mean64 (means over 64 ceil(C / 64)), swap_gb (dgamma and dbeta exchanged)
    spec mask: nyquist2 (the Nyquist column doubled, even W), last1 (the last column not doubled, odd W)
    avgpool adjoint: fill_odd (the odd last row filled)
    attention backward: dk_twice (0.25 applied to dk twice), nomax (softmax without the maximum subtraction: must fail on the
           large-logit cases)
"""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import train_ref as R  # noqa: E402

f32 = np.float32

# (family, mutant) -> why the assertion cannot see it
UNDETECTABLE = {
    ("unary", "relu:x>=0"): "selects x itself at x = +-0, which is the value 0 either way",
    ("unary", "softplus:x>=20"): "log1p(exp(20)) = 20 + 2.1e-9 rounds to 20 in fp32: both branches return the same float",
    ("unary", "softplus_bwd:x>=20"): "sigmoid(20) = 1 - 2.1e-9 rounds to 1 in fp32: both branches return g",
}
WORST = {}


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)


def seq_sum(a, axis):
    """Strictly sequential fp32 sum along an axis."""
    return np.add.accumulate(a, axis=axis, dtype=f32).take(-1, axis=axis)


def expect_fail(family, mutant, case, got, ref, mag, c, floor=0.0, undetected=None):
    if R.passes(got, ref, mag, c, floor) and (family, mutant) not in UNDETECTABLE:
        undetected.append(f"{family}:{mutant}@{case}")


# ---------------------------------------------------------------------------------------------------------------------
# weight gradients
def wgrad_plan(B, H, W, Cin, Cout, KH, KW):
    """csrc/train_ops.hip conv_wgrad_refactor + conv_wgrad_plan: the geometry the kernel walks and its rows per chunk."""
    if KH == 1 and KW == 1:
        M = B * H * W
        for cand in (512, 256, 128, 64, 32, 16, 8):
            if M % cand == 0:
                B, H, W = 1, M // cand, cand
                break
    MI = 2 if Cout > 32 else 1
    njobs = -(-Cout // (32 * MI)) * -(-Cin // 32) * KH * KW
    nrows = B * H
    want = max(1, min(-(-2048 // njobs), (nrows + 3) // 4))
    rpc = -(-nrows // want)
    return B, H, W, rpc, -(-nrows // rpc)


def wgrad_standin(case, x, dz, dw0, mut=None):
    B, H, W, Cin, Cout, KH, KW = case
    B, H, W, rpc, nchunks = wgrad_plan(*case)
    x, dz = x.reshape(B, H, W, Cin), dz.reshape(B, H, W, Cout).copy()
    if mut == "last_col":
        dz[:, :, W - 1] = 0
    if mut == "tail8":
        dz[:, :, (W // 8) * 8:] = 0
    if mut == "last_chunk":
        dz.reshape(B * H, W, Cout)[(nchunks - 1) * rpc:] = 0
    if mut == "chan":
        if Cin % 32 and Cin > 1:
            x = x.copy()
            x[..., Cin - 1] = x[..., Cin - 2]
        else:
            dz[..., Cout - 1] = dz[..., Cout - 2]
    out = np.zeros((Cout, KH * KW, Cin), f32)
    for ky in range(KH):
        for kx in range(KW):
            oy, ox = ky - KH // 2, kx - KW // 2
            if mut == "swap_kykx":
                oy, ox = kx - KW // 2, ky - KH // 2
            if mut == "pad":
                ox -= 1
            xs = R.shifted(x, oy, ox, prev_image=mut == "prev_image").reshape(-1, 1, Cin)
            prod = dz.reshape(-1, Cout, 1) * xs
            out[:, ky * KW + kx] = np.add.accumulate(prod, axis=0, out=prod)[-1]
    out = out.reshape(Cout, -1)
    return out if dw0 is None or mut == "no_acc" else dw0 + out


def wgrad_mutants(case, acc):
    B, H, W, Cin, Cout, KH, KW = case
    gW = wgrad_plan(*case)[2]
    m = ["last_col", "last_chunk", "pad"]
    if gW % 8:
        m.append("tail8")
    if KH * KW > 1 and (KH != KW or H != W):
        m.append("swap_kykx")
    if B > 1 and KH > 1:
        m.append("prev_image")
    if acc:
        m.append("no_acc")
    if (Cin % 32 and Cin > 1) or (Cout % 32 and Cout > 1):
        m.append("chan")
    return m


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_wgrad_reference(case):
    B, H, W, Cin, Cout, KH, KW = case
    x, dz, dw0, w = R.wgrad_inputs(case)
    undetected = []
    base = {m: wgrad_standin(case, x, dz, None, m) for m in [None] + [m for m in wgrad_mutants(case, False)]}
    for acc in (False, True):
        ref, mag = R.conv_wgrad_ref(x, dz, KH, KW, dw0 if acc else None)
        note("wgrad", R.check(base[None] + dw0 if acc else base[None], ref, mag, R.C_WGRAD, f"stand-in {case} acc={acc}"))
        for m in wgrad_mutants(case, acc):
            got = base[None] if m == "no_acc" else (base[m] + dw0 if acc else base[m])
            expect_fail("wgrad", m, case, got, ref, mag, R.C_WGRAD, undetected=undetected)
    assert not undetected, undetected
    # the references are the gradients of F.conv2d
    xt, wt = (torch.from_numpy(R.f64(a)).requires_grad_(True) for a in (x, w))
    w4 = wt.reshape(Cout, KH, KW, Cin).permute(0, 3, 1, 2)
    bt = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xt.permute(0, 3, 1, 2), w4, bt, padding=(KH // 2, KW // 2)).permute(0, 2, 3, 1)
    y.backward(torch.from_numpy(R.f64(dz)))
    for got, (ref, mag) in ((wt.grad, R.conv_wgrad_ref(x, dz, KH, KW)), (xt.grad, R.conv_dgrad_ref(dz, w, KH, KW)), (bt.grad, R.bias_grad_ref(dz))):
        assert (np.abs(got.numpy() - ref) <= 1e-12 * mag).all()
    # dx and db stand-ins: the same sequential fp32 sums
    ref, mag = R.bias_grad_ref(dz)
    note("reduce", R.check(seq_sum(dz.reshape(-1, Cout), 0), ref, mag, R.C_REDUCE, f"db {case}"))
    if (B * H * W) * Cout * Cin * KH * KW <= 4e7:
        ref, mag = R.conv_dgrad_ref(dz, w, KH, KW)
        w3 = w.reshape(Cout, KH * KW, Cin)
        terms = np.stack([R.shifted(dz, -(ky - KH // 2), -(kx - KW // 2)).reshape(-1, Cout)[:, :, None] * w3[None, :, ky * KW + kx]
                          for ky in range(KH) for kx in range(KW)], 1).reshape(B * H * W, -1, Cin)
        note("wgrad", R.check(seq_sum(terms, 1).reshape(B, H, W, Cin), ref, mag, R.C_WGRAD, f"dx {case}"))


def dwgrad_standin(x, dy, KH, KW, dw0):
    C = x.shape[-1]
    out = np.zeros((KH * KW, C), f32)
    for ky in range(KH):
        for kx in range(KW):
            out[ky * KW + kx] = seq_sum((dy * R.shifted(x, ky - KH // 2, kx - KW // 2)).reshape(-1, C), 0)
    return out if dw0 is None else dw0 + out


@pytest.mark.parametrize("k", R.DW_KERNELS, ids=lambda k: f"{k[0]}x{k[1]}")
@pytest.mark.parametrize("case", R.DWGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dwconv_wgrad_reference(case, k):
    x, dy, dw0 = R.dwgrad_inputs(case, k)
    C = case[3]
    for acc in (None, dw0):
        ref, mag = R.dwconv_wgrad_ref(x, dy, k[0], k[1], acc)
        note("dwgrad", R.check(dwgrad_standin(x, dy, k[0], k[1], acc), ref, mag, R.C_DWGRAD, f"stand-in {case} {k}"))
    xt = torch.from_numpy(R.f64(x)).requires_grad_(True)
    wt = torch.from_numpy(R.f64(dw0)).requires_grad_(True)                     # [taps, C]
    y = F.conv2d(xt.permute(0, 3, 1, 2), wt.t().reshape(C, 1, k[0], k[1]), None, padding=(k[0] // 2, k[1] // 2), groups=C)
    y.backward(torch.from_numpy(R.f64(dy)).permute(0, 3, 1, 2))
    ref, mag = R.dwconv_wgrad_ref(x, dy, k[0], k[1])
    assert (np.abs(wt.grad.numpy() - ref) <= 1e-12 * mag).all()


# ---------------------------------------------------------------------------------------------------------------------
# column and row sums
def reduce_cols_standin(x, y, y_kind, rpg, scale, out0, mut=None):
    rows, C = x.shape
    rpg = rpg or rows
    if mut == "y_col" and y_kind == 1:
        y = np.broadcast_to(y[np.minimum(np.arange(C), rows - 1), 0][None, :], (rows, C))
    p = (x if y is None else x * y).astype(f32)
    if mut == "shift":
        p = np.concatenate([p[1:], np.zeros((1, C), f32)])
    p = p.reshape(rows // rpg, rpg, C).copy()
    if mut == "last_row":
        p[:, -1] = 0
    s = seq_sum(p, 1) * f32(scale)
    if mut == "scale2":
        s = s * f32(scale)
    return s if out0 is None else out0 + s


@pytest.mark.parametrize("case", R.REDUCE_COLS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_reduce_cols_reference(case):
    rows, C, rpg = case
    undetected = []
    for y_kind in R.REDUCE_COLS_YKINDS:
        x, y = R.reduce_inputs(rows, C, y_kind)
        out0 = R.draw(5, rows // (rpg or rows), C)
        for acc in (None, out0):
            ref, mag = R.reduce_cols_ref(x, y, rpg, R.REDUCE_SCALE, acc)
            note("reduce", R.check(reduce_cols_standin(x, y, y_kind, rpg, R.REDUCE_SCALE, acc), ref, mag, R.C_REDUCE, f"cols {case} y{y_kind}"))
            for m in ["last_row", "scale2"] + (["shift"] if rows > 1 else []) + (["y_col"] if y_kind == 1 and rows > 1 else []):
                expect_fail("reduce", m, (case, y_kind), reduce_cols_standin(x, y, y_kind, rpg, R.REDUCE_SCALE, acc, m), ref, mag, R.C_REDUCE,
                            undetected=undetected)
        xt = torch.from_numpy(R.f64(x))
        tref = R.REDUCE_SCALE * (xt if y is None else xt * torch.from_numpy(R.f64(y))).reshape(-1, rpg or rows, C).sum(1)
        ref, mag = R.reduce_cols_ref(x, y, rpg, R.REDUCE_SCALE)
        assert (np.abs(tref.numpy() - ref) <= 1e-12 * mag).all()
    assert not undetected, undetected


@pytest.mark.parametrize("case", R.REDUCE_ROWS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_reduce_rows_reference(case):
    rows, C = case
    undetected = []
    for y_kind in R.REDUCE_ROWS_YKINDS:
        x, y = R.reduce_inputs(rows, C, y_kind)
        out0 = R.draw(5, rows)
        p = (x if y is None else x * y).astype(f32)
        for acc in (None, out0):
            ref, mag = R.reduce_rows_ref(x, y, R.REDUCE_SCALE, acc)
            fin = lambda s: s if acc is None else acc + s
            note("reduce", R.check(fin(seq_sum(p, 1) * f32(R.REDUCE_SCALE)), ref, mag, R.C_REDUCE, f"rows {case} y{y_kind}"))
            expect_fail("reduce", "scale2", (case, y_kind), fin(seq_sum(p, 1) * f32(R.REDUCE_SCALE) * f32(R.REDUCE_SCALE)), ref, mag, R.C_REDUCE,
                        undetected=undetected)
            expect_fail("reduce", "last_col", (case, y_kind), fin((seq_sum(p, 1) - p[:, -1]) * f32(R.REDUCE_SCALE)), ref, mag, R.C_REDUCE,
                        undetected=undetected)
        xt = torch.from_numpy(R.f64(x))
        tref = R.REDUCE_SCALE * (xt if y is None else xt * torch.from_numpy(R.f64(y))).sum(1)
        ref, mag = R.reduce_rows_ref(x, y, R.REDUCE_SCALE)
        assert (np.abs(tref.numpy() - ref) <= 1e-12 * mag).all()
    assert not undetected, undetected


def flat_sum_standin(terms):
    """l1_stage1_kernel / sqnorm_stage1_kernel + sum_finish_kernel: grid-stride terms per thread, LDS trees, 256-thread finish."""
    def tree(v):
        h = 128
        while h:
            v = v[..., :h] + v[..., h:2 * h]
            h //= 2
        return v[..., 0]
    n = terms.size
    nb = min(1024, -(-n // 256))
    per = -(-n // (256 * nb))
    t = np.zeros(per * nb * 256, f32)
    t[:n] = terms
    part = tree(seq_sum(t.reshape(per, nb, 256), 0))
    p = np.zeros(-(-nb // 256) * 256, f32)
    p[:nb] = part
    return tree(seq_sum(p.reshape(-1, 256), 0))


def test_l1_sqnorm_reference():
    for n in R.FLAT_NS:
        sr, hr = R.l1_inputs(n)
        loss, mag, dsr = R.l1_loss_grad_ref(sr, hr)
        inv_n = f32(1.0) / f32(n)
        got = flat_sum_standin(np.abs(np.clip(sr, f32(0), f32(1)) - hr)) * inv_n
        print(f"l1 {n}: stand-in {R.check(np.array([got]), loss, mag, R.c_flat_sum(n), f'l1 {n}'):.2f} of {R.c_flat_sum(n)}")
        assert not R.passes(np.array([got * inv_n]), loss, mag, R.c_flat_sum(n)) or n == 1, "l1: scale applied twice undetected"
        st = torch.from_numpy(R.f64(sr)).requires_grad_(True)
        lt = (st.clamp(0, 1) - torch.from_numpy(R.f64(hr))).abs().mean()
        lt.backward()
        assert abs(lt.item() * n * float(inv_n) - loss[0]) <= 1e-12 * mag[0]
        assert (np.abs(st.grad.numpy() * n - dsr / float(inv_n)) <= 1e-12).all()
        g = R.draw(7, n, scale=0.01)
        ref, mag = R.sqnorm_ref(g)
        R.check(np.array([flat_sum_standin(g * g)]), ref, mag, R.c_flat_sum(n), f"sqnorm {n}")


# ---------------------------------------------------------------------------------------------------------------------
# pointwise
def test_ew_fma_reference():
    rows, rpg = R.EW_FMA_ROWS, R.EW_FMA_RPG
    for C in R.EW_FMA_CS:
        a = R.draw(1, rows, C)
        for bk, ck in R.EW_FMA_KINDS:
            b, c = R.fma_operand(bk, rows, C, rpg, 2), R.fma_operand(ck, rows, C, rpg, 3)
            for av in (a, None):
                for clamp in (0, 1):
                    ref, mag = R.ew_fma_ref(av, b, bk, c, ck, R.EW_FMA_SCALE, rows, C, rpg, clamp)
                    ex = lambda t, k, absent: R._expand(t, k, rows, C, rpg, absent).astype(f32)
                    got = (av if av is not None else f32(1)) * ex(b, bk, 1.0)
                    if ck != 4:
                        got = got + f32(R.EW_FMA_SCALE) * ex(c, ck, 0.0)
                    if clamp:
                        got = np.clip(got, f32(0), f32(1))
                    R.check(got, ref, mag, R.C_EW_FMA, f"fma C={C} b{bk} c{ck}")
                    if clamp == 0 and av is not None:                       # the broadcast rules, written with torch's own
                        tt = lambda t, k, absent: torch.full((rows, C), absent, dtype=torch.float64) if k == 4 else (
                            torch.from_numpy(R.f64(t)).repeat_interleave(rpg, dim=0) if k == 2 else torch.from_numpy(R.f64(t)).expand(rows, C))
                        tref = torch.from_numpy(R.f64(av)) * tt(b, bk, 1.0) + float(f32(R.EW_FMA_SCALE)) * tt(c, ck, 0.0)
                        assert (np.abs(tref.numpy() - ref) <= 1e-12 * mag).all()


def unary_standin(name, x, g, p0, mut=None):
    """csrc/train_ops.hip ew_unary_apply in torch fp32.  mut: "<op>:<changed comparison>"."""
    x, g = torch.from_numpy(x), (torch.from_numpy(g) if g is not None else None)
    p0, one, zero = f32(p0), torch.ones(()), torch.zeros(())
    m = (mut or "").split(":")[-1]
    gt = (lambda a, b: a >= b) if m in ("x>=0", "x>=20") else (lambda a, b: a > b)
    sig = lambda t: 1.0 / (1.0 + torch.exp(-t)) if m == "notail" else torch.where(t < -87.0, torch.exp(t), 1.0 / (1.0 + torch.exp(-t)))
    if name == "gelu":
        r = 0.5 * x * (1.0 + torch.erf(x * f32(0.70710678118654752440)))
    elif name == "relu":
        r = torch.where(gt(x, 0.0), x, zero)
    elif name == "sigmoid":
        r = sig(x)
    elif name == "softplus":
        r = torch.where(gt(x, 20.0), x, torch.log1p(torch.exp(x)))
    elif name == "abs":
        r = x.abs()
    elif name == "clamp01":
        r = x.clamp(0.0, 1.0)
    elif name == "scale":
        r = x * p0
    elif name == "recip_eps":
        r = 1.0 / (x + p0)
    elif name == "clamp_min":
        r = torch.maximum(x, torch.tensor(p0))
    elif name == "exp":
        r = torch.exp(x)
    elif name == "gelu_bwd":
        cdf = 0.5 * (1.0 + torch.erf(x * f32(0.70710678118654752440)))
        r = g * (cdf + x * (f32(0.39894228040143267794) * torch.exp(-0.5 * x * x)))
    elif name == "relu_bwd":
        r = torch.where(gt(x, 0.0), g, zero)
    elif name == "sigmoid_bwd_y":
        y = sig(x) if m == "fed_x" else x
        r = g * y * (1.0 - y)
    elif name == "softplus_bwd":
        r = torch.where(gt(x, 20.0), g, torch.where((x < -87.0) & (m != "notail"), g * torch.exp(x), g / (1.0 + torch.exp(-x))))
    elif name == "abs_bwd":
        pos = x >= 0 if m == "sgn0=1" else x > 0
        neg = x <= 0 if m == "x<=0" else x < 0
        r = torch.where(pos, g, torch.where(neg, -g, zero))
    elif name == "clamp01_bwd":
        lo = x > 0 if m == "x>0" else x >= 0
        hi = x < 1 if m == "x<1" else x <= 1
        r = torch.where(lo & hi, g, zero)
    elif name == "recip_bwd":
        r = -g * x * x
    elif name == "clamp_min_bwd":
        r = torch.where(x > p0 if m == "x>p0" else x >= p0, g, zero)
    elif name == "exp_bwd_y":
        r = g * x
    return r.numpy()


UNARY_MUTANTS = ["relu:x>=0", "relu_bwd:x>=0", "softplus:x>=20", "softplus_bwd:x>=20", "abs_bwd:sgn0=1", "abs_bwd:x<=0", "clamp01_bwd:x>0",
                 "clamp01_bwd:x<1", "clamp_min_bwd:x>p0", "sigmoid_bwd_y:fed_x", "sigmoid:notail", "softplus_bwd:notail"]


def test_ew_unary_reference():
    x, g = R.unary_vector()
    assert x.dtype == f32 and g.dtype == f32
    for name, (_, count, has_g) in R.UNARY.items():
        ref, mag = R.unary_ref(name, x, g if has_g else None)
        r = R.unary_check(name, unary_standin(name, x, g if has_g else None, R.UNARY_P0), ref, mag, f"stand-in {name}")
        print(f"unary {name}: stand-in worst {r:.2f} of {count}")
    undetected = []
    for mut in UNARY_MUTANTS:
        name = mut.split(":")[0]
        has_g = R.UNARY[name][2]
        ref, mag = R.unary_ref(name, x, g if has_g else None)
        got = unary_standin(name, x, g if has_g else None, R.UNARY_P0, mut)
        hit = R.passes(got, ref, mag, R.UNARY[name][1], R.FLT_MIN)
        if hit and ("unary", mut) not in UNDETECTABLE:
            undetected.append(mut)
        assert hit or ("unary", mut) not in UNDETECTABLE, f"{mut} is listed as undetectable but is detected"
    assert not undetected, undetected
    # the forms that take the OUTPUT y: torch autograd at y = f(z)
    z = torch.from_numpy(R.f64(x).clip(-30, 30)).requires_grad_(True)
    gt = torch.from_numpy(R.f64(g))
    for name, f in (("sigmoid_bwd_y", torch.sigmoid), ("exp_bwd_y", torch.exp), ("recip_bwd", lambda t: 1.0 / (t + 40.0))):
        z.grad = None
        y = f(z)
        y.backward(gt)
        ref, mag = R.unary_ref(name, y.detach().numpy(), g)
        assert (np.abs(z.grad.numpy() - ref) <= 1e-12 * np.maximum(mag, R.FLT_MIN)).all(), name


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
def ln_standin(x, dy, gamma, eps, dgb0, mut=None):
    C = x.shape[1]
    n = f32(64 * -(-C // 64) if mut == "mean64" else C)
    mean = seq_sum(x, 1)[:, None] / n
    d = x - mean
    rstd = f32(1) / np.sqrt(seq_sum(d * d, 1)[:, None] / n + f32(eps))
    xh, gh = d * rstd, dy * gamma
    m1, m2 = seq_sum(gh, 1)[:, None] / n, seq_sum(gh * xh, 1)[:, None] / n
    dx = rstd * (gh - m1 - xh * m2)
    dgb = np.stack([seq_sum(dy * xh, 0), seq_sum(dy, 0)])
    if mut == "swap_gb":
        dgb = dgb[::-1].copy()
    return dx, (dgb if dgb0 is None else dgb0 + dgb)


@pytest.mark.parametrize("case", R.LN_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]:g}-{c[3]:g}")
def test_layernorm_bwd_reference(case):
    rows, C, eps, shift = case
    x, dy, gamma = R.ln_inputs(case)
    dgb0 = R.draw(9, 2, C)
    undetected = []
    for acc in (None, dgb0):
        dx, dxm, dgb, dgbm = R.layernorm_bwd_ref(x, dy, gamma, eps, acc)
        sdx, sdgb = ln_standin(x, dy, gamma, eps, acc)
        note("ln_bwd", R.check(sdx, dx, dxm, R.C_LN_BWD, f"dx {case}"))
        note("ln_bwd", R.check(sdgb, dgb, dgbm, R.C_LN_BWD, f"dgamma|dbeta {case}"))
        for m in ["swap_gb"] + (["mean64"] if C % 64 else []):
            mdx, mdgb = ln_standin(x, dy, gamma, eps, acc, m)
            if R.passes(mdx, dx, dxm, R.C_LN_BWD) and R.passes(mdgb, dgb, dgbm, R.C_LN_BWD):
                undetected.append(f"ln_bwd:{m}@{case}")
    assert not undetected, undetected
    if rows <= 700:
        xt, gt = (torch.from_numpy(R.f64(a)).requires_grad_(True) for a in (x, gamma))
        bt = torch.zeros(C, dtype=torch.float64, requires_grad=True)
        F.layer_norm(xt, (C,), gt, bt, float(f32(eps))).backward(torch.from_numpy(R.f64(dy)))
        dx, dxm, dgb, dgbm = R.layernorm_bwd_ref(x, dy, gamma, eps)
        assert (np.abs(xt.grad.numpy() - dx) <= 1e-12 * dxm).all()
        assert (np.abs(np.stack([gt.grad.numpy(), bt.grad.numpy()]) - dgb) <= 1e-12 * dgbm).all()


# ---------------------------------------------------------------------------------------------------------------------
# average-pool adjoint, FFT mask
@pytest.mark.parametrize("hw", R.AVGPOOL_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_avgpool2_adj_reference(hw):
    H, W = hw
    undetected = []
    for C in (1, 5):
        dy, dx0 = R.draw(1, 2, H // 2, W // 2, C), R.draw(2, 2, H, W, C)
        for acc in (None, dx0):
            ref, mag = R.avgpool2_adj_ref(dy, H, W, acc)
            up = np.zeros((2, H, W, C), f32)
            up[:, :2 * (H // 2), :2 * (W // 2)] = f32(0.25) * np.repeat(np.repeat(dy, 2, 1), 2, 2)
            R.check(up if acc is None else acc + up, ref, mag, R.C_AVGPOOL_ADJ, f"avgpool adj {hw}")
            if H % 2:
                up[:, H - 1] = up[:, H - 2]
                expect_fail("avgpool", "fill_odd", hw, up if acc is None else acc + up, ref, mag, R.C_AVGPOOL_ADJ, undetected=undetected)
        xt = torch.from_numpy(R.f64(dx0)).requires_grad_(True)
        F.avg_pool2d(xt.permute(0, 3, 1, 2), 2, 2).backward(torch.from_numpy(R.f64(dy)).permute(0, 3, 1, 2))
        ref, mag = R.avgpool2_adj_ref(dy, H, W)
        assert (np.abs(xt.grad.numpy() - ref) <= 1e-12 * mag).all()
    assert not undetected, undetected


def spec_grad_standin(gY, X, W, dm0, mut=None):
    planes, H, Wf, _ = X.shape
    s = seq_sum(gY[..., 0] * X[..., 0] + gY[..., 1] * X[..., 1], 0)            # per plane re re + im im, as the kernel sums them
    kx = np.arange(Wf)
    hi = (W - 1) // 2
    if mut == "nyquist2":
        hi = W // 2
    if mut == "last1":
        hi = (W - 1) // 2 - 1
    s = s * np.where((kx >= 1) & (kx <= hi), f32(2), f32(1))[None, :]
    return s if dm0 is None else dm0 + s


@pytest.mark.parametrize("hw", R.SPEC_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_spec_mask_reference(hw):
    H, W = hw
    undetected = []
    for planes in R.SPEC_PLANES:
        X, gY, m, x, g = R.spec_inputs(H, W, planes)
        ref, mag = R.spec_mask_mul_ref(X, m)
        R.check(X * m[None, :, :, None], ref, mag, R.C_SPEC_MUL, f"spec mul {hw}")
        dm0 = R.draw(4, H, W // 2 + 1)
        for acc in (None, dm0):
            ref, mag = R.spec_mask_grad_ref(gY, X, W, acc)
            note("reduce", R.check(spec_grad_standin(gY, X, W, acc), ref, mag, R.C_REDUCE, f"spec grad {hw}"))
            mut = "last1" if W % 2 else "nyquist2"
            expect_fail("spec", mut, (hw, planes), spec_grad_standin(gY, X, W, acc, mut), ref, mag, R.C_REDUCE, undetected=undetected)
        # dm of sum(g * irfft2(rfft2(x) * m)) by fp64 autograd
        mt = torch.from_numpy(R.f64(m)).requires_grad_(True)
        xt, gt = torch.from_numpy(x), torch.from_numpy(g)
        torch.fft.irfft2(torch.fft.rfft2(xt, norm="ortho") * mt, s=(H, W), norm="ortho").backward(gt)
        st = lambda z: np.stack([z.real, z.imag], -1)
        ref, mag = R.spec_mask_grad_ref(st(np.fft.rfft2(g, norm="ortho")), st(np.fft.rfft2(x, norm="ortho")), W)
        assert (np.abs(mt.grad.numpy() - ref) <= 1e-12 * np.maximum(mag, 1e-300)).all()
    assert not undetected, undetected


# ---------------------------------------------------------------------------------------------------------------------
# attention core
def mha_standin(qkv, dout, P, nt, heads, mut=None):
    E = heads * 16
    t = qkv.reshape(P, nt, 3, heads, 16)
    q, k, v = (np.ascontiguousarray(t[:, :, i].transpose(0, 2, 1, 3)) for i in range(3))
    go = np.ascontiguousarray(dout.reshape(P, nt, heads, 16).transpose(0, 2, 1, 3))
    qs = q * f32(0.25)
    s, dp = np.zeros((P, heads, nt, nt), f32), np.zeros((P, heads, nt, nt), f32)
    for d in range(16):
        s = s + qs[:, :, :, None, d] * k[:, :, None, :, d]
        dp = dp + go[:, :, :, None, d] * v[:, :, None, :, d]
    mx = np.zeros_like(s[..., :1]) if mut == "nomax" else s.max(-1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(s - mx)
        w = e / seq_sum(e, 3)[..., None]
        out = np.zeros((P, heads, nt, 16), f32)
        for j in range(nt):
            out = out + v[:, :, None, j] * w[:, :, :, j, None]
        dot = seq_sum(dp * w, 3)[..., None]
        ds = w * (dp - dot) * f32(0.25)
        dq, dk, dv = (np.zeros((P, heads, nt, 16), f32) for _ in range(3))
        for j in range(nt):
            dq = dq + k[:, :, None, j] * ds[:, :, :, j, None]
        for i in range(nt):
            dk = dk + q[:, :, None, i] * ds[:, :, i, :, None]
            dv = dv + go[:, :, None, i] * w[:, :, i, :, None]
        if mut == "dk_twice":
            dk = dk * f32(0.25)
    rows = lambda a: a.transpose(0, 2, 1, 3).reshape(P * nt, E)
    return rows(out), np.concatenate([rows(dq), rows(dk), rows(dv)], 1)


@pytest.mark.parametrize("case", R.MHA_CASES, ids=lambda c: f"nt{c[0]}-h{c[1]}-P{c[2]}-s{c[3]:g}")
def test_band_mha_reference(case):
    nt, heads, P, scale = case
    qkv, dout = R.mha_inputs(case)
    out, outm, dqkv, dqkvm = R.band_mha_ref(qkv, dout, P, nt, heads)
    so, sd = mha_standin(qkv, dout, P, nt, heads)
    note("mha", R.check(so, out, outm, R.C_MHA_BWD, f"out {case}"))
    note("mha", R.check(sd, dqkv, dqkvm, R.C_MHA_BWD, f"dqkv {case}"))
    undetected = []
    for m in ["dk_twice"] + (["nomax"] if R.mha_max_logit(qkv, P, nt, heads) > 89.0 else []):      # expf overflows above 88.7
        mo, md = mha_standin(qkv, dout, P, nt, heads, m)
        if R.passes(mo, out, outm, R.C_MHA_BWD) and R.passes(md, dqkv, dqkvm, R.C_MHA_BWD):
            undetected.append(f"mha:{m}@{case}")
    assert not undetected, undetected
    E = heads * 16
    qt = torch.from_numpy(R.f64(qkv)).requires_grad_(True)
    q, k, v = [u.reshape(P, nt, heads, 16).transpose(1, 2) for u in qt.chunk(3, dim=-1)]
    a = (torch.softmax((q * 0.25) @ k.transpose(-2, -1), dim=-1) @ v).transpose(1, 2).reshape(P * nt, E)
    a.backward(torch.from_numpy(R.f64(dout)))
    assert (np.abs(a.detach().numpy() - out) <= 1e-12 * outm).all()
    assert (np.abs(qt.grad.numpy() - dqkv) <= 1e-12 * dqkvm).all()


def test_exact_movement_references():
    for A, Bd, C in R.PERMUTE_CASES:
        x = torch.arange(A * Bd * C, dtype=torch.float32)
        assert np.array_equal(R.permute_rows_ref(x.numpy(), A, Bd, C), x.reshape(A, Bd, C).transpose(0, 1).contiguous().numpy())
    for Cout, Cin, KH, KW in R.FLIPT_CASES:
        w = R.draw(1, Cout, KH * KW * Cin)
        wt = R.conv_weight_flipT_ref(w, Cout, Cin, KH * KW).reshape(Cin, KH * KW * Cout)
        dz = R.draw(2, 1, 5, 4, Cout)
        # conv(dz, wt) with the same padding is the data gradient
        z = F.conv2d(torch.from_numpy(R.f64(dz)).permute(0, 3, 1, 2), torch.from_numpy(R.f64(wt)).reshape(Cin, KH, KW, Cout).permute(0, 3, 1, 2),
                     None, padding=(KH // 2, KW // 2)).permute(0, 2, 3, 1)
        ref, mag = R.conv_dgrad_ref(dz, w, KH, KW)
        assert (np.abs(z.numpy() - ref) <= 1e-12 * mag).all()


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm (training mode), bilinear adjoint, AdamW + EMA
def bn_standin(i, G):
    """The tape's batchnorm_train and its backward in fp32, column sums strictly sequential."""
    x, dy, gamma, beta = i["x"], i["dy"], i["gamma"], i["beta"]
    C = x.shape[1]
    n = x.shape[0] // G
    xg, dyg, nf = x.reshape(G, n, C), dy.reshape(G, n, C), f32(n)
    s1 = seq_sum(xg, 1)
    xc = xg - (s1 * f32(1.0 / n))[:, None]
    s2 = seq_sum(xc * xc, 1)
    mean, var = s1 / nf, np.maximum(s2 / nf, f32(0))
    rstd = f32(1) / np.sqrt(var + f32(R.BN_EPS))
    sc = gamma * rstd
    y = xg * sc[:, None] + (beta - mean * sc)[:, None]
    rm, rv, mo = i["rm0"].copy(), i["rv0"].copy(), f32(R.BN_MOMENTUM)
    for g in range(G):
        rm = (f32(1) - mo) * rm + mo * mean[g]
        rv = (f32(1) - mo) * rv + mo * (var[g] * nf / (nf - f32(1)) if n > 1 else var[g])
    xh = (xg - mean[:, None]) * rstd[:, None]
    sdy, sdyxh, inv = seq_sum(dyg, 1), seq_sum(dyg * xh, 1), f32(1) / nf
    dx = (gamma * rstd)[:, None] * (dyg - (sdy * inv)[:, None] - xh * (sdyxh * inv)[:, None])
    return dict(y=y.reshape(-1, C), running_mean=rm, running_var=rv, dx=dx.reshape(-1, C), dgamma=seq_sum(sdyxh, 0), dbeta=seq_sum(sdy, 0))


@pytest.mark.parametrize("case", R.BN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_batchnorm_train_reference(case):
    G, C, rpg = case
    i = R.bn_inputs(case)
    ref = R.batchnorm_train_ref(i["x"], i["gamma"], i["beta"], i["rm0"], i["rv0"], i["dy"], G)
    for k, v in bn_standin(i, G).items():
        note("bn_bwd" if R.BN_CONST[k] == "C_BN_BWD" else "bn_stat", R.check(v, *ref[k], getattr(R, R.BN_CONST[k]), f"bn {k} {case}"))
    xt, gt, bt = (torch.from_numpy(R.f64(i[k])).requires_grad_(True) for k in ("x", "gamma", "beta"))
    rm, rv = torch.from_numpy(R.f64(i["rm0"])), torch.from_numpy(R.f64(i["rv0"]))
    y = torch.cat([F.batch_norm(xt[g * rpg:(g + 1) * rpg], rm, rv, gt, bt, True, float(f32(R.BN_MOMENTUM)), float(f32(R.BN_EPS))) for g in range(G)])
    y.backward(torch.from_numpy(R.f64(i["dy"])))
    for k, t in (("y", y.detach()), ("dx", xt.grad), ("dgamma", gt.grad), ("dbeta", bt.grad), ("running_mean", rm), ("running_var", rv)):
        assert (np.abs(t.numpy() - ref[k][0]) <= 1e-12 * ref[k][1]).all(), k


def bn_finish_standin(i, centered, n):
    s1, s2, gamma, beta, nf, mo = i["s1"], i["s2"], i["gamma"], i["beta"], f32(n), f32(R.BN_MOMENTUM)
    mean = s1 / nf
    var = np.maximum(s2 / nf if centered else s2 / nf - mean * mean, f32(0))
    rstd = f32(1) / np.sqrt(var + f32(R.BN_EPS))
    sc = gamma * rstd
    rm, rv = i["rm0"].copy(), i["rv0"].copy()
    for g in range(s1.shape[0]):
        rm = (f32(1) - mo) * rm + mo * mean[g]
        rv = (f32(1) - mo) * rv + mo * (var[g] * nf / (nf - f32(1)) if n > 1 else var[g])
    return dict(mean_rstd=np.stack([mean, rstd], -1), scale=sc, shift=beta - mean * sc, running_mean=rm, running_var=rv)


@pytest.mark.parametrize("case", R.BN_FINISH_CASES, ids=lambda c: "-".join(f"{v:g}" for v in c))
def test_bn_finish_reference(case):
    G, C, n, shift, scale = case
    for centered in (0, 1):
        i = R.bn_finish_inputs(case, centered)
        ref = R.bn_finish_ref(i["s1"], i["s2"], centered, n, i["gamma"], i["beta"], i["rm0"], i["rv0"])
        for k, v in bn_finish_standin(i, centered, n).items():
            R.check(v, *ref[k], R.C_BN_FINISH, f"bn finish {k} {case} centered={centered}")
    # against F.batch_norm on the data the centred sums came from (exact sums): the same statistics
    x = torch.from_numpy(R.f64(R.draw(1, G, n, C, scale=scale, shift=shift)))
    i = R.bn_finish_inputs(case, 1)
    ref = R.bn_finish_ref(x.sum(1).numpy(), ((x - x.mean(1, keepdim=True)) ** 2).sum(1).numpy(), 1, n, i["gamma"], i["beta"], i["rm0"], i["rv0"])
    rm, rv = torch.from_numpy(R.f64(i["rm0"])), torch.from_numpy(R.f64(i["rv0"]))
    if n > 1:
        ys = [F.batch_norm(x[g], rm, rv, torch.from_numpy(R.f64(i["gamma"])), torch.from_numpy(R.f64(i["beta"])), True, float(f32(R.BN_MOMENTUM)),
                           float(f32(R.BN_EPS))) for g in range(G)]
        y = torch.stack(ys).numpy()
        mine = x.numpy() * ref["scale"][0][:, None] + ref["shift"][0][:, None]
        assert (np.abs(y - mine) <= 1e-11 * (np.abs(x.numpy() * ref["scale"][0][:, None]) + np.abs(ref["shift"][0][:, None]) + 1.0)).all()
        assert (np.abs(rm.numpy() - ref["running_mean"][0]) <= 1e-12 * ref["running_mean"][1]).all()
        assert (np.abs(rv.numpy() - ref["running_var"][0]) <= 1e-12 * ref["running_var"][1]).all()


def resize_adj_standin(dy, Hi, Wi, sh, sw, mul, dx0):
    Ay, Ax = R.resize_axis(Hi, dy.shape[1], f32(sh), f32)[0], R.resize_axis(Wi, dy.shape[2], f32(sw), f32)[0]
    rs = seq_sum(Ax[None, None, :, :, None] * dy[:, :, None, :, :], 3)                   # [B, Ho, Wi, C], sequential over ox
    s = seq_sum(Ay[None, :, :, None, None] * rs[:, None], 2) * f32(mul)                  # [B, Hi, Wi, C], sequential over oy
    return s if dx0 is None else dx0 + s


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_resize_adj_reference(case):
    Hi, Wi, Ho, Wo, sf = case
    for C in (1, 5):
        dy, dx0 = R.draw(1, 2, Ho, Wo, C), R.draw(2, 2, Hi, Wi, C)
        sh, sw = R.aten_scale(Hi, Ho, sf), R.aten_scale(Wi, Wo, sf)
        for acc in (None, dx0):
            ref, mag = R.resize_adj_ref(dy, Hi, Wi, sh, sw, R.RESIZE_MUL, acc)
            note("resize", R.check(resize_adj_standin(dy, Hi, Wi, sh, sw, R.RESIZE_MUL, acc), ref, mag, R.C_RESIZE_ADJ, f"resize adj {case}"))
        xt = torch.from_numpy(R.f64(dx0)).requires_grad_(True)
        kw = dict(scale_factor=sf) if sf else dict(size=(Ho, Wo))
        yt = F.interpolate(xt.permute(0, 3, 1, 2), mode="bilinear", align_corners=False, **kw)
        assert tuple(yt.shape[2:]) == (Ho, Wo)
        (yt * R.RESIZE_MUL).backward(torch.from_numpy(R.f64(dy)).permute(0, 3, 1, 2))
        ref, mag = R.resize_adj_ref(dy, Hi, Wi, R.aten_scale(Hi, Ho, sf, np.float64), R.aten_scale(Wi, Wo, sf, np.float64), R.RESIZE_MUL)
        assert (np.abs(xt.grad.numpy() - ref) <= 1e-12 * mag).all()


def adamw_standin(i, hyper, sqnorm, with_ema):
    lr, b1, b2, eps, wd, max_norm, decay, _, step_size, bc2s = (f32(v) for v in hyper)
    coef = min(max_norm / (np.sqrt(f32(sqnorm)) + f32(1e-6)), f32(1)) if max_norm > 0 else f32(1)
    gi = i["g"] * coef
    pi = i["p"] * (f32(1) - lr * wd)
    mi = i["m"] + (gi - i["m"]) * (f32(1) - b1)
    vi = i["v"] * b2 + (f32(1) - b2) * gi * gi
    pi = pi - step_size * (mi / (np.sqrt(vi) / bc2s + eps))
    out = dict(g=gi, m=mi, v=vi, p=pi)
    if with_ema:
        out["ema"] = decay * i["ema"] + (f32(1) - decay) * pi
    return out


def test_adamw_ema_reference():
    for n in R.FLAT_NS:
        i = R.adamw_inputs(n)
        sq = float((R.f64(i["g"]) ** 2).sum())
        for max_norm in (1e3, 0.5 * math.sqrt(sq), 0.0):                      # clip inactive, active, off
            hyper = R.adamw_hyper(max_norm)
            for with_ema in (True, False):
                ref = R.adamw_ema_ref(i["p"], i["g"], i["m"], i["v"], i["ema"] if with_ema else None, hyper, f32(sq))
                for k, v in adamw_standin(i, hyper, sq, with_ema).items():
                    R.check(v, *ref[k], R.C_ADAMW, f"adamw {k} n={n} max_norm={max_norm:g}", floor=R.FLT_MIN)
            if max_norm > 0:                                                  # torch.optim.AdamW + clip_grad_norm_ in fp64, unrounded hyper
                h = R.ADAMW_HYPER
                pt = torch.nn.Parameter(torch.from_numpy(R.f64(i["p"])))
                opt = torch.optim.AdamW([pt], lr=h["lr"], betas=(h["b1"], h["b2"]), weight_decay=h["wd"], eps=h["eps"])
                opt.state[pt] = dict(step=torch.tensor(float(h["step"] - 1)), exp_avg=torch.from_numpy(R.f64(i["m"])),
                                     exp_avg_sq=torch.from_numpy(R.f64(i["v"])))
                pt.grad = torch.from_numpy(R.f64(i["g"]))
                torch.nn.utils.clip_grad_norm_([pt], max_norm)
                opt.step()
                ref = R.adamw_ema_ref(i["p"], i["g"], i["m"], i["v"], None, R.adamw_hyper(max_norm, np.float64), sq)
                for k, t in (("p", pt.data), ("m", opt.state[pt]["exp_avg"]), ("v", opt.state[pt]["exp_avg_sq"]), ("g", pt.grad)):
                    assert (np.abs(t.numpy() - ref[k][0]) <= 1e-11 * ref[k][1]).all(), (k, n, max_norm)


def dft_tables(n):
    ang = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    return np.cos(ang).astype(f32), np.sin(ang).astype(f32)


def cols_standin(a, b, sign):
    """cdft_cols_kernel: [C, H, Wf] re / im -> the DFT over H with e^{sign i theta}, sequential over h."""
    H = a.shape[1]
    ch, sh = dft_tables(H)
    idx = (np.arange(H)[:, None] * np.arange(H)[None, :]) % H                   # [kh, h]
    cs, sn = ch[idx][None, :, :, None], (f32(sign) * sh)[idx][None, :, :, None]
    nrm = f32(1) / np.sqrt(f32(H))
    return (seq_sum(a[:, None] * cs - b[:, None] * sn, 2) * nrm, seq_sum(a[:, None] * sn + b[:, None] * cs, 2) * nrm)


def rfft2_standin(x):
    W = x.shape[2]
    Wf = W // 2 + 1
    cw, sw = dft_tables(W)
    idx = (np.arange(Wf)[:, None] * np.arange(W)[None, :]) % W                  # [k, n]
    nrm = f32(1) / np.sqrt(f32(W))
    re, im = cols_standin(seq_sum(x[:, :, None, :] * cw[idx], 3) * nrm, -seq_sum(x[:, :, None, :] * sw[idx], 3) * nrm, -1.0)
    return np.stack([re, im], -1)


def irfft2_standin(spec, W):
    ure, uim = cols_standin(spec[..., 0], spec[..., 1], 1.0)                    # [C, H, Wf]
    cw, sw = dft_tables(W)
    w = np.arange(W)
    s = np.broadcast_to(ure[:, :, :1], ure.shape[:2] + (W,)).copy()
    if W % 2 == 0:
        s = s + np.where(w % 2, f32(-1), f32(1)) * ure[:, :, W // 2:W // 2 + 1]
    for k in range(1, (W - 1) // 2 + 1):
        idx = (k * w) % W
        s = s + f32(2) * (ure[:, :, k:k + 1] * cw[idx] - uim[:, :, k:k + 1] * sw[idx])
    return s * (f32(1) / np.sqrt(f32(W)))


@pytest.mark.parametrize("hw", R.SPEC_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_dft_reference(hw):
    H, W = hw
    for planes in R.SPEC_PLANES:
        x = R.draw(21, planes, H, W)
        ref, mag = R.rfft2_ref(x)
        note("dft", R.check(rfft2_standin(x), ref, mag, R.C_DFT, f"rfft2 {hw}"))
        zt = torch.view_as_real(torch.fft.rfft2(torch.from_numpy(R.f64(x)), norm="ortho")).numpy()
        assert (np.abs(zt - ref) <= 1e-12 * mag).all()
        spec = R.spec_inputs(H, W, planes)[0] * R.draw(22, H, W // 2 + 1)[None, :, :, None]      # a masked spectrum: imaginary DC column and all
        ref, mag = R.irfft2_ref(spec, W)
        note("dft", R.check(irfft2_standin(spec, W), ref, mag, R.C_DFT, f"irfft2 {hw}"))
        zt = torch.fft.irfft2(torch.view_as_complex(torch.from_numpy(R.f64(spec))), s=(H, W), norm="ortho").numpy()
        assert (np.abs(zt - ref) <= 1e-12 * mag).all()


# ---------------------------------------------------------------------------------------------------------------------
def test_zz_measured_constants():
    """Runs last in this module (file order): the worst stand-in ratios per family against the recorded *_MEASURED values."""
    need = {"wgrad": R.C_WGRAD_MEASURED, "dwgrad": R.C_DWGRAD_MEASURED, "reduce": R.C_REDUCE_MEASURED, "ln_bwd": R.C_LN_BWD_MEASURED,
            "mha": R.C_MHA_BWD_MEASURED, "bn_stat": R.C_BN_STAT_MEASURED, "bn_bwd": R.C_BN_BWD_MEASURED, "resize": R.C_RESIZE_ADJ_MEASURED, "dft": R.C_DFT_MEASURED}
    if set(need) - set(WORST):
        pytest.skip("measured over the whole module: run the file, not a selection")
    for fam, meas in need.items():
        print(f"TRAIN_REF_MEASURED {fam}: {WORST[fam]:.3f} (recorded {meas})")
    for fam, meas in need.items():
        assert WORST[fam] <= 1.25 * meas, (fam, WORST[fam], meas)
        assert WORST[fam] >= meas / 4.0, (fam, WORST[fam], meas, "the recorded value is far above what is measured")
    for c, meas in ((R.C_WGRAD, R.C_WGRAD_MEASURED), (R.C_DWGRAD, R.C_DWGRAD_MEASURED), (R.C_REDUCE, R.C_REDUCE_MEASURED),
                    (R.C_LN_BWD, R.C_LN_BWD_MEASURED), (R.C_MHA_BWD, R.C_MHA_BWD_MEASURED), (R.C_BN_BWD, R.C_BN_BWD_MEASURED),
                    (R.C_BN_STAT, R.C_BN_STAT_MEASURED),
                    (R.C_RESIZE_ADJ, R.C_RESIZE_ADJ_MEASURED), (R.C_DFT, R.C_DFT_MEASURED)):
        assert c == 4.0 * meas
