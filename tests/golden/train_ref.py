"""fp64 references and per-element error bounds for the training kernels of csrc/train_ops.hip (pure numpy / torch, no GPU).

Every reference returns `ref` (fp64) and `mag` (fp64), both per element.  `mag` is the sum of the absolute values of the terms that
make up the element -- sum |dz| |x| for a weight gradient, |a b| + |s c| for a multiply-add -- and the assertion is per element,
never per tensor maximum:

    |kernel - ref| <= C_op * 2^-24 * mag                                    (check())

An element whose mag is 0 (a tap that only ever reads padding) must come back exactly 0; a reference value beyond the fp32 range must
come back as the same infinity.

Constants of the reductions (C_WGRAD, C_DWGRAD, C_REDUCE, C_LN_BWD, C_MHA_BWD, C_BN_STAT, C_BN_BWD, C_RESIZE_ADJ, C_DFT).  None was fitted to a kernel's output.  Each is
MEASURED on the CPU by tests/test_train_ref_cpu.py: a stand-in plays the kernel's arithmetic with a strictly sequential fp32
accumulation (np.add.accumulate in float32) of the same fp32 products, in pixel order -- the worst of the orders the kernels use, which
split the same sum over at least 4 chains and a fixed tree -- and the largest |stand-in - ref| / (2^-24 mag) over the case tables below
is recorded as *_MEASURED.  The kernels are held to REDUCTION_FACTOR = 4 times that, the factor stage_ref.GEMM_NOISE_FACTOR uses for
"the same fp32 sum in another order".  The CPU test repeats the measurement and asserts that it stays within 1.25 * MEASURED.

The loss and squared-norm sums (n up to 262147 terms of one sign) are the exception: their constant, c_flat_sum(n), is DERIVED from the
kernels' fixed tree, where the others are measured.  C_ADAMW and the pointwise budgets below are derived as well.

Conditioning.  Where a kernel subtracts a mean or a maximum before it multiplies, the terms of mag carry the magnitude of the operands
of that subtraction, not of its result:
    layernorm_bwd   the difference x - mean is off by a multiple of 2^-24 (|x| + |mean|), and rstd by the relative kappa = mean_c(|xh| xm),
                    xm = (|x| + |mean|) rstd (1 for centred rows, ~100 for x = 100 + noise).  So xh = (x - mean) rstd carries the mag
                    xhm = xm + |xh| kappa, and dx = rstd (gh - m1 - xh m2) the terms rstd (|gh| + mean|gh| + |xh| mean|gh xh|), what
                    xh's own error moves, rstd (xhm |m2| + |xh| mean(|gh| xhm)), and kappa |dx| for the factor rstd;
    band_mha        the softmax weights carry the factor (1 + L_i), L_i = max_j 0.25 sum_d |q_id k_jd| the magnitude of the logits'
                    terms: an fp32 logit is off by a multiple of 2^-24 L_i, and exp turns that into a relative error of the weight;
                    plus FLT_MIN, since a weight far below the row's largest (which is exactly 1 before the division) underflows.

Rounding budgets of the pointwise kernels, counted instruction by instruction (units of 2^-24 relative to the stated magnitude; a
correctly rounded operation costs 1, a library function its documented ulp bound times 2: expf 1 ulp, erff 4 ulp, log1pf 2 ulp; fp32
division is correctly rounded).  Below FLT_MIN the fp32 spacing is 2^-149 = 2 * 2^-24 * FLT_MIN, so the pointwise bounds use
max(mag, FLT_MIN): that is the format's precision, not a floor on the scale of the data.
    ew_fma           3 on |a b| + |c_scale c|        two products and one sum (at most two roundings reach one term)
    gelu             8 on |x|            t = x c: 1 (0.5 after erf' t <= 0.5) + c's own rounding 0.5; erff 8; 1 + erf: 2 -> 11 on the
                                         factor (1 + erf) <= 2, halved by 0.5 x: 5.5; the product: 1.  Largest intermediate |x|.
    sigmoid          4 on |y|            expf 2, 1 + e 1, division 1 (x < -87: expf alone, 2)
    softplus         6 on |y|            expf 2 (e / ((1 + e) log1p e) <= 1), log1pf 4; x > 20: exact
    scale            1 on |x p0|
    recip_eps        2 on |y|            the sum x + p0 1, division 1
    exp              2 on |y|
    gelu_bwd         8 on |g| (1 + |x| phi(x))   cdf: 5.5 (as above); x x: 1 -> at most 0.25 through x phi(x) x^2 / 2; expf 2, its
                                         constant 1, x pdf 1: 4 on |x| phi; the sum 1; g (...) 1.  Largest intermediate 1 + erf.
    sigmoid_bwd_y    3 on |g y (1 - y)|  1 - y, two products
    softplus_bwd     4 on |g sigmoid(x)| as sigmoid with g in the numerator; x > 20: exact
    recip_bwd        2 on |g y^2|
    exp_bwd_y        1 on |g y|
    relu, abs, clamp01, clamp_min and their derivative forms: 0 (selections and sign changes are exact)
    avgpool2_adj     1 on |0.25 dy| + |dx0|  (the accumulate's sum; 0.25 dy is exact)
    spec_mask_mul    1 on |X m|
    l1 gradient      0: +-fp32(1 / n), selected
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
FLT_MIN = 2.0 ** -126
REDUCTION_FACTOR = 4.0

# measured by tests/test_train_ref_cpu.py with the sequential fp32 stand-ins over the case tables of this module
C_WGRAD_MEASURED = 5.8
C_DWGRAD_MEASURED = 3.6
C_REDUCE_MEASURED = 4.7
C_LN_BWD_MEASURED = 3.3
C_MHA_BWD_MEASURED = 2.7
C_WGRAD = REDUCTION_FACTOR * C_WGRAD_MEASURED
C_DWGRAD = REDUCTION_FACTOR * C_DWGRAD_MEASURED
C_REDUCE = REDUCTION_FACTOR * C_REDUCE_MEASURED
C_LN_BWD = REDUCTION_FACTOR * C_LN_BWD_MEASURED
C_MHA_BWD = REDUCTION_FACTOR * C_MHA_BWD_MEASURED

C_EW_FMA = 3.0
C_AVGPOOL_ADJ = 1.0
C_SPEC_MUL = 1.0


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the assertion
def draw(seed, *shape, scale=1.0, shift=0.0):
    """Seeded N(0, 1) * scale + shift as float32."""
    return (np.random.default_rng(seed).standard_normal(shape) * scale + shift).astype(np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def ratios(got, ref, mag, floor=0.0):
    """|got - ref| / (2^-24 mag) per element: 0 where both vanish, inf where got differs and mag is 0 or got is not finite.
    Where ref overflows fp32 the kernel must return that infinity (ratio 0) or anything else (ratio inf)."""
    got, ref, mag = f64(got), f64(ref), np.maximum(f64(mag), floor)
    assert got.shape == ref.shape == mag.shape, (got.shape, ref.shape, mag.shape)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ref32 = ref.astype(np.float32).astype(np.float64)
        big = ~np.isfinite(ref32)
        d = np.abs(got - np.where(big, 0.0, ref))
        r = np.where(d == 0.0, 0.0, d / (U24 * mag))
        r = np.where(np.isfinite(got), r, np.inf)
        r = np.where(big, np.where(got == ref32, 0.0, np.inf), r)
    return r


def check(got, ref, mag, c, what, floor=0.0):
    """Per-element assertion; returns the worst ratio seen (for the reports)."""
    r = ratios(got, ref, mag, floor)
    worst = float(r.max()) if r.size else 0.0
    if not worst <= c:
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError(f"{what}: |d| / (2^-24 mag) = {worst:.3g} > {c:g} at {i}: got {f64(got)[i]!r}, ref {f64(ref)[i]!r}, "
                             f"mag {f64(mag)[i]!r}; {int((r > c).sum())} of {r.size} elements over")
    return worst


def passes(got, ref, mag, c, floor=0.0):
    r = ratios(got, ref, mag, floor)
    return bool((r <= c).all())


# ---------------------------------------------------------------------------------------------------------------------
# convolution weight / data / bias gradients
# (B, H, W, Cin, Cout, KH, KW)
WGRAD_CASES = [(1, 3, 8, 3, 1, 3, 3), (1, 5, 13, 33, 65, 3, 3), (3, 7, 9, 31, 33, 3, 3), (2, 2, 3, 32, 32, 3, 3), (1, 1, 5, 4, 4, 3, 3),
               (2, 20, 20, 73, 64, 3, 3), (1, 9, 50, 27, 3, 3, 3), (2, 6, 11, 8, 40, 1, 3), (2, 11, 6, 8, 40, 3, 1), (1, 6, 7, 5, 6, 5, 5),
               (1, 1, 1003, 27, 64, 1, 1), (1, 1, 1000, 64, 3, 1, 1), (2, 16, 16, 96, 32, 1, 1), (3, 7, 9, 33, 33, 1, 1)]
WGRAD_SPATIAL = [c for c in WGRAD_CASES if c[5] * c[6] > 1]


def wgrad_inputs(case, seed=0):
    B, H, W, Cin, Cout, KH, KW = case
    return (draw(seed + 1, B, H, W, Cin), draw(seed + 2, B, H, W, Cout), draw(seed + 3, Cout, KH * KW * Cin, scale=0.5),
            draw(seed + 4, Cout, KH * KW * Cin, scale=0.2))          # x, dz, the dw an accumulate adds to, a weight for dx


def shifted(x, oy, ox, prev_image=False):
    """out[b, y, x] = x[b, y + oy, x + ox], zero outside the image.  prev_image (a mutant of the CPU test): a row above an image's
    first row is read from the previous image's last rows."""
    B, H, W, C = x.shape
    out = np.zeros_like(x)
    ys, xs = np.arange(H), np.arange(W)
    vy, vx = (ys + oy >= 0) & (ys + oy < H), (xs + ox >= 0) & (xs + ox < W)
    if vy.any() and vx.any():
        out[np.ix_(np.arange(B), ys[vy], xs[vx])] = x[np.ix_(np.arange(B), (ys + oy)[vy], (xs + ox)[vx])]
    if prev_image and oy < 0 and vx.any():
        fo, fi = out.reshape(B * H, W, C), x.reshape(B * H, W, C)
        r = np.arange(B * H)
        rr = r[((r % H) + oy < 0) & (r + oy >= 0)]
        if rr.size:
            fo[np.ix_(rr, xs[vx])] = fi[np.ix_(rr + oy, (xs + ox)[vx])]
    return out


def conv_wgrad_ref(x, dz, KH, KW, dw0=None):
    """dW[co][tap * Cin + ci] = sum_{b,y,x} dz[b,y,x,co] in[b, y+ky-py, x+kx-px, ci] (+ dw0)."""
    x, dz = f64(x), f64(dz)
    Cin, Cout = x.shape[-1], dz.shape[-1]
    ref, mag = np.zeros((Cout, KH * KW, Cin)), np.zeros((Cout, KH * KW, Cin))
    za = np.abs(dz).reshape(-1, Cout)
    for ky in range(KH):
        for kx in range(KW):
            xs = shifted(x, ky - KH // 2, kx - KW // 2).reshape(-1, Cin)
            ref[:, ky * KW + kx] = dz.reshape(-1, Cout).T @ xs
            mag[:, ky * KW + kx] = za.T @ np.abs(xs)
    ref, mag = ref.reshape(Cout, -1), mag.reshape(Cout, -1)
    if dw0 is not None:
        ref, mag = ref + f64(dw0), mag + np.abs(f64(dw0))
    return ref, mag


def conv_dgrad_ref(dz, w, KH, KW):
    """dx[b,Y,X,ci] = sum_{ky,kx,co} dz[b, Y-ky+py, X-kx+px, co] w[co][tap][ci]; w packed [Cout, KH*KW*Cin]."""
    dz, w = f64(dz), f64(w)
    B, H, W, Cout = dz.shape
    w = w.reshape(Cout, KH * KW, -1)
    Cin = w.shape[-1]
    ref, mag = np.zeros((B * H * W, Cin)), np.zeros((B * H * W, Cin))
    for ky in range(KH):
        for kx in range(KW):
            zs = shifted(dz, -(ky - KH // 2), -(kx - KW // 2)).reshape(-1, Cout)
            ref += zs @ w[:, ky * KW + kx]
            mag += np.abs(zs) @ np.abs(w[:, ky * KW + kx])
    return ref.reshape(B, H, W, Cin), mag.reshape(B, H, W, Cin)


def bias_grad_ref(dz):
    dz = f64(dz).reshape(-1, dz.shape[-1])
    return dz.sum(0), np.abs(dz).sum(0)


# (B, H, W, C) x kernels; (3, 90, 5, 130) walks more than 64 chunks
DWGRAD_CASES = [(1, 4, 5, 3), (3, 7, 9, 65), (2, 24, 28, 64), (3, 90, 5, 130)]
DW_KERNELS = [(3, 3), (5, 5), (1, 21), (21, 1)]


def dwgrad_inputs(case, k, seed=0):
    B, H, W, C = case
    return draw(seed + 1, B, H, W, C), draw(seed + 2, B, H, W, C), draw(seed + 3, k[0] * k[1], C, scale=0.5)


def dwconv_wgrad_ref(x, dy, KH, KW, dw0=None):
    """dw[tap][c] = sum_{b,y,x} dy[b,y,x,c] in[b, y+ky-py, x+kx-px, c] (+ dw0)."""
    x, dy = f64(x), f64(dy)
    C = x.shape[-1]
    ref, mag = np.zeros((KH * KW, C)), np.zeros((KH * KW, C))
    for ky in range(KH):
        for kx in range(KW):
            p = dy * shifted(x, ky - KH // 2, kx - KW // 2)
            ref[ky * KW + kx], mag[ky * KW + kx] = p.reshape(-1, C).sum(0), np.abs(p).reshape(-1, C).sum(0)
    if dw0 is not None:
        ref, mag = ref + f64(dw0), mag + np.abs(f64(dw0))
    return ref, mag


# ---------------------------------------------------------------------------------------------------------------------
# column / row sums.  y_kind as in the C ABI: 0 full, 1 per row, 2 per column, 4 absent
# (rows, C, rows_per_group)
REDUCE_COLS_CASES = [(1030, c, 0) for c in (1, 3, 9, 27, 48, 64, 65, 76, 130, 200)] + \
    [(1, 9, 0), (7, 64, 0), (511, 3, 0), (513, 65, 0), (40000, 9, 0), (600, 27, 2), (4000, 3, 2), (3078, 76, 1026)]
REDUCE_COLS_YKINDS = (0, 1, 4)
# (rows, C)
REDUCE_ROWS_CASES = [(r, c) for c in (1, 16, 17, 64, 65, 200) for r in (1, 1000)] + [(70000, 17)]
REDUCE_ROWS_YKINDS = (0, 2, 4)
REDUCE_SCALE = 0.37


def reduce_inputs(rows, C, y_kind, seed=0):
    x = draw(seed + 1, rows, C)
    y = {0: lambda: draw(seed + 2, rows, C), 1: lambda: draw(seed + 2, rows, 1), 2: lambda: draw(seed + 2, 1, C), 4: lambda: None}[y_kind]()
    return x, y


def _prod(x, y):
    return f64(x) if y is None else f64(x) * f64(y)           # y broadcasts: [rows, C], [rows, 1] or [1, C]


def reduce_cols_ref(x, y, rpg, scale, out0=None):
    """out[g][c] = scale * sum over the rows of group g of x (* y) (+ out0)."""
    p = _prod(x, y)
    rows, C = p.shape
    rpg = rpg or rows
    p = p.reshape(rows // rpg, rpg, C)
    ref, mag = scale * p.sum(1), abs(scale) * np.abs(p).sum(1)
    if out0 is not None:
        ref, mag = ref + f64(out0), mag + np.abs(f64(out0))
    return ref, mag


def reduce_rows_ref(x, y, scale, out0=None):
    """out[r] = scale * sum_c x (* y) (+ out0)."""
    p = _prod(x, y)
    ref, mag = scale * p.sum(1), abs(scale) * np.abs(p).sum(1)
    if out0 is not None:
        ref, mag = ref + f64(out0), mag + np.abs(f64(out0))
    return ref, mag


# ---------------------------------------------------------------------------------------------------------------------
# a * b + s * c with broadcast operands: kind 0 full, 1 per row, 2 per (group, column), 3 scalar, 4 absent
EW_FMA_ROWS, EW_FMA_RPG, EW_FMA_CS = 1030, 103, (1, 9, 65)
EW_FMA_KINDS = [(bk, ck) for bk in range(5) for ck in range(5)]
EW_FMA_SCALE = -0.37


def fma_operand(kind, rows, C, rpg, seed):
    shape = {0: (rows, C), 1: (rows, 1), 2: (rows // rpg, C), 3: (1,)}.get(kind)
    return None if shape is None else draw(seed, *shape)


def _expand(t, kind, rows, C, rpg, absent):
    if kind == 4 or t is None:
        return np.full((rows, C), absent)
    t = f64(t)
    if kind == 2:
        return np.repeat(t, rpg, axis=0)
    return np.broadcast_to(t.reshape(1, 1) if kind == 3 else t, (rows, C))


def ew_fma_ref(a, b, b_kind, c, c_kind, c_scale, rows, C, rpg, clamp01):
    ab = (f64(a) if a is not None else 1.0) * _expand(b, b_kind, rows, C, rpg, 1.0)
    sc = float(np.float32(c_scale)) * _expand(c, c_kind, rows, C, rpg, 0.0)
    ref = ab + sc
    if clamp01:
        ref = np.clip(ref, 0.0, 1.0)                    # exact and 1-Lipschitz: the unclamped bound carries over
    return ref, np.abs(ab) + np.abs(sc)


# ---------------------------------------------------------------------------------------------------------------------
# the 19 unary forms: name -> (op code of the C ABI, rounding count, takes a gradient).  Budgets: the module docstring.
UNARY = dict(gelu=(0, 8, False), relu=(1, 0, False), sigmoid=(2, 4, False), softplus=(3, 6, False), abs=(4, 0, False), clamp01=(5, 0, False),
             scale=(6, 1, False), recip_eps=(7, 2, False), clamp_min=(8, 0, False), exp=(9, 2, False),
             gelu_bwd=(16, 8, True), relu_bwd=(17, 0, True), sigmoid_bwd_y=(18, 3, True), softplus_bwd=(19, 4, True), abs_bwd=(20, 0, True),
             clamp01_bwd=(21, 0, True), recip_bwd=(22, 2, True), clamp_min_bwd=(23, 0, True), exp_bwd_y=(24, 1, True))
UNARY_P0 = float(np.float32(0.3))
_FWD = dict(gelu=F.gelu, relu=F.relu, sigmoid=torch.sigmoid, softplus=F.softplus, abs=torch.abs, clamp01=lambda t: t.clamp(0.0, 1.0),
            exp=torch.exp)
_BWD_OF = dict(gelu_bwd="gelu", relu_bwd="relu", softplus_bwd="softplus", abs_bwd="abs", clamp01_bwd="clamp01", clamp_min_bwd="clamp_min")


def unary_vector(p0=UNARY_P0, seed=11, draws=4096):
    """The special points of the 19 forms (fp32), then seeded N(0, 1) * 3 draws; with a gradient of the same length (never 0)."""
    f = np.float32
    na = lambda v, d: np.nextafter(f(v), f(d))
    pts = [0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 1e-4, -1e-4, 0.5, -0.5, 1.0, -1.0, na(1, np.inf), na(1, -np.inf), na(-1, np.inf),
           na(-1, -np.inf), 20.0, na(20, np.inf), na(20, -np.inf), 5.0, -5.0, 10.0, -10.0, 30.0, -30.0, 87.0, -87.0, 100.0, -100.0,
           p0, na(p0, np.inf), na(p0, -np.inf), -p0, na(0, np.inf), na(0, -np.inf)]
    x = np.concatenate([np.array(pts, dtype=f), draw(seed, draws, scale=3.0)])
    g = draw(seed + 1, x.size)
    g = np.where(np.abs(g) < 0.05, f(0.7), g).astype(f)
    return x, g


def unary_ref(name, x, g, p0=UNARY_P0):
    """(ref, mag).  The derivative forms of x come from torch fp64 autograd of the torch function they mirror, so torch's tie rules are
    the reference: clamp bounds inclusive, sgn(0) = 0, relu'(0) = 0, softplus threshold 20."""
    xt = torch.from_numpy(f64(x).copy())
    gt = torch.from_numpy(f64(g).copy()) if g is not None else None
    fwd = dict(_FWD, scale=lambda t: t * p0, recip_eps=lambda t: 1.0 / (t + p0), clamp_min=lambda t: t.clamp(min=p0))
    if name in fwd:
        ref = fwd[name](xt)
    elif name in _BWD_OF:
        xt.requires_grad_(True)
        fwd[_BWD_OF[name]](xt).backward(gt)
        ref = xt.grad
        xt = xt.detach()
    elif name == "sigmoid_bwd_y":
        ref = gt * xt * (1.0 - xt)
    elif name == "recip_bwd":
        ref = -gt * xt * xt
    elif name == "exp_bwd_y":
        ref = gt * xt
    else:
        raise KeyError(name)
    ref, xa = ref.numpy(), np.abs(xt.numpy())
    if name == "gelu":
        mag = xa
    elif name == "gelu_bwd":
        mag = np.abs(f64(g)) * (1.0 + xa * np.exp(-0.5 * xa * xa) / math.sqrt(2.0 * math.pi))
    else:
        mag = np.abs(ref)
    return ref, mag


def unary_check(name, got, ref, mag, what=""):
    return check(got, ref, mag, UNARY[name][1], what or name, floor=FLT_MIN)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
LN_CS = (3, 63, 64, 65, 128, 200, 256)
LN_ROWS = (1, 3, 65, 700)
# (rows, C, eps, shift): the cross of LN_CS x LN_ROWS at eps 1e-5, every C at 65 rows with eps 1e-6, the nblk cap, x = 100 + noise
LN_CASES = [(r, c, 1e-5, 0.0) for c in LN_CS for r in LN_ROWS] + [(65, c, 1e-6, 0.0) for c in LN_CS] + \
    [(131077, 64, 1e-5, 0.0), (700, 65, 1e-5, 100.0)]


def ln_inputs(case, seed=0):
    rows, C, eps, shift = case
    return draw(seed + 1, rows, C, shift=shift), draw(seed + 2, rows, C), draw(seed + 3, C, scale=0.2, shift=1.0)      # x, dy, gamma


def layernorm_bwd_ref(x, dy, gamma, eps, dgb0=None):
    """dx [rows, C] and dgamma | dbeta [2, C] (+ dgb0), with their mags (conditioning: the module docstring)."""
    x, dy, gamma = f64(x), f64(dy), f64(gamma)
    eps = float(np.float32(eps))
    mean = x.mean(1, keepdims=True)
    d = x - mean
    rstd = 1.0 / np.sqrt((d * d).mean(1, keepdims=True) + eps)
    xh, gh = d * rstd, dy * gamma
    m1, m2 = gh.mean(1, keepdims=True), (gh * xh).mean(1, keepdims=True)
    dx = rstd * (gh - m1 - xh * m2)
    xm = (np.abs(x) + np.abs(mean)) * rstd
    kappa = np.maximum((np.abs(xh) * xm).mean(1, keepdims=True), 1.0)
    xhm = xm + np.abs(xh) * kappa
    gha, xha = np.abs(gh), np.abs(xh)
    dx_mag = rstd * (gha + gha.mean(1, keepdims=True) + xha * (gha * xha).mean(1, keepdims=True) + xhm * np.abs(m2)
                     + xha * (gha * xhm).mean(1, keepdims=True)) + kappa * np.abs(dx)
    dgb = np.stack([(dy * xh).sum(0), dy.sum(0)])
    dgb_mag = np.stack([(np.abs(dy) * xhm).sum(0), np.abs(dy).sum(0)])
    if dgb0 is not None:
        dgb, dgb_mag = dgb + f64(dgb0), dgb_mag + np.abs(f64(dgb0))
    return dx, dx_mag, dgb, dgb_mag


# ---------------------------------------------------------------------------------------------------------------------
# adjoint of avg_pool2d(2)
AVGPOOL_CASES = [(2, 3), (3, 2), (31, 30), (9, 9)]


def avgpool2_adj_ref(dy, H, W, dx0=None):
    """dx[b,y,x,c] = 0.25 dy[b, y/2, x/2, c] inside 2 (H/2) x 2 (W/2), 0 on an odd last row / column (+ dx0)."""
    dy = f64(dy)
    B, Ho, Wo, C = dy.shape
    assert (Ho, Wo) == (H // 2, W // 2)
    ref = np.zeros((B, H, W, C))
    ref[:, :2 * Ho, :2 * Wo] = 0.25 * np.repeat(np.repeat(dy, 2, axis=1), 2, axis=2)
    mag = np.abs(ref)
    if dx0 is not None:
        ref, mag = ref + f64(dx0), mag + np.abs(f64(dx0))
    return ref, mag


# ---------------------------------------------------------------------------------------------------------------------
# the FFT mask product and its mask gradient on half spectra [planes][H][Wf][2]
SPEC_CASES = [(5, 7), (9, 15), (17, 8), (2, 2), (24, 40)]
SPEC_PLANES = (1, 6)


def spec_inputs(H, W, planes, seed=0):
    """Half spectra (ortho) of seeded real images, rounded to fp32: X of the input, gY of the incoming gradient; the mask m."""
    x, g = f64(draw(seed + 1, planes, H, W)), f64(draw(seed + 2, planes, H, W))
    as_f32 = lambda z: np.stack([z.real, z.imag], -1).astype(np.float32)
    m = 1.0 / (1.0 + np.exp(-f64(draw(seed + 3, H, W // 2 + 1))))
    return as_f32(np.fft.rfft2(x, norm="ortho")), as_f32(np.fft.rfft2(g, norm="ortho")), m.astype(np.float32), x, g


def spec_mask_mul_ref(X, m):
    ref = f64(X) * f64(m)[None, :, :, None]
    return ref, np.abs(ref)


def spec_mask_grad_ref(gY, X, W, dm0=None):
    """dm[ky][kx] = f(kx) sum_planes Re(gY conj X), f = 2 for the columns with a conjugate partner (1 <= kx <= (W - 1) / 2; the
    Nyquist column of an even W has none), else 1."""
    p = f64(gY) * f64(X)                                         # [planes, H, Wf, 2]: re re, im im
    Wf = p.shape[2]
    kx = np.arange(Wf)
    f = np.where((kx >= 1) & (kx <= (W - 1) // 2), 2.0, 1.0)[None, :]
    ref, mag = f * p.sum((0, 3)), f * np.abs(p).sum((0, 3))
    if dm0 is not None:
        ref, mag = ref + f64(dm0), mag + np.abs(f64(dm0))
    return ref, mag


# ---------------------------------------------------------------------------------------------------------------------
# the 3- / 9-token attention core (d = 16 per head, q scaled by 0.25), forward and backward, no dropout
# (ntok, heads, P, input scale): scale 8 gives logits of a few hundred, where the maximum subtraction matters
MHA_CASES = [(nt, h, p, s) for nt in (3, 9) for h in (1, 4, 8) for p in (1, 37) for s in (1.0, 8.0)]


def mha_inputs(case, seed=0):
    nt, heads, P, s = case
    E = heads * 16
    return draw(seed + 1, P * nt, 3 * E, scale=s), draw(seed + 2, P * nt, E)


def band_mha_ref(qkv, dout, P, nt, heads):
    """-> out, out_mag [P*nt, E], dqkv, dqkv_mag [P*nt, 3E]."""
    E = heads * 16
    t = f64(qkv).reshape(P, nt, 3, heads, 16)
    q, k, v = (t[:, :, i].transpose(0, 2, 1, 3) for i in range(3))          # [P, heads, nt, 16]
    go = f64(dout).reshape(P, nt, heads, 16).transpose(0, 2, 1, 3)
    s = 0.25 * np.einsum("phid,phjd->phij", q, k)
    L = 0.25 * np.einsum("phid,phjd->phij", np.abs(q), np.abs(k)).max(-1, keepdims=True)       # [P, heads, nt, 1]
    w = np.exp(s - s.max(-1, keepdims=True))
    w /= w.sum(-1, keepdims=True)
    wm = w * (1.0 + L) + FLT_MIN                  # the largest exp is exactly 1; one far below it underflows in fp32 (spacing 2^-149)
    out = np.einsum("phij,phjd->phid", w, v)
    out_mag = np.einsum("phij,phjd->phid", wm, np.abs(v))
    dp = np.einsum("phid,phjd->phij", go, v)
    dpm = np.einsum("phid,phjd->phij", np.abs(go), np.abs(v))
    ds = 0.25 * w * (dp - (dp * w).sum(-1, keepdims=True))
    dsm = 0.25 * wm * (dpm + (dpm * wm).sum(-1, keepdims=True))
    dq, dqm = np.einsum("phij,phjd->phid", ds, k), np.einsum("phij,phjd->phid", dsm, np.abs(k))
    dk, dkm = np.einsum("phij,phid->phjd", ds, q), np.einsum("phij,phid->phjd", dsm, np.abs(q))
    dv, dvm = np.einsum("phij,phid->phjd", w, go), np.einsum("phij,phid->phjd", wm, np.abs(go))
    rows = lambda a: a.transpose(0, 2, 1, 3).reshape(P * nt, E)
    cat = lambda a, b, c: np.concatenate([rows(a), rows(b), rows(c)], 1)
    return rows(out), rows(out_mag), cat(dq, dk, dv), cat(dqm, dkm, dvm)


def mha_max_logit(qkv, P, nt, heads):
    t = f64(qkv).reshape(P, nt, 3, heads, 16)
    return float((0.25 * np.einsum("pihd,pjhd->phij", t[:, :, 0], t[:, :, 1])).max())


# ---------------------------------------------------------------------------------------------------------------------
# L1 loss and gradient, squared norm
FLAT_NS = (1, 255, 257, 262147)


def l1_inputs(n, seed=0):
    """sr with exact 0, exact 1, values outside [0, 1] and entries equal to hr; hr in [0, 1]."""
    sr = draw(seed + 1, n, scale=0.6, shift=0.5)
    hr = np.random.default_rng(seed + 2).random(n, dtype=np.float32)
    for i, v in enumerate((0.0, 1.0, -0.25, 1.5)):
        if 4 + i < n:
            sr[4 + i] = v
    if n > 16:
        hr[4], hr[5] = 0.0, 1.0                                   # d = 0 at the inclusive bounds
        sr[9:13] = hr[9:13]
    return sr, hr


def l1_loss_grad_ref(sr, hr):
    """loss = mean |clamp(sr, 0, 1) - hr| with its mag, and dsr = sign(clamp(sr) - hr) * fp32(1 / n) inside [0, 1], else 0 (exact)."""
    s, h = f64(sr), f64(hr)
    n = s.size
    d = np.clip(s, 0.0, 1.0) - h
    inv_n = float(np.float32(1.0) / np.float32(n))
    loss, mag = np.abs(d).sum() * inv_n, (np.abs(np.clip(s, 0.0, 1.0)) + np.abs(h)).sum() * inv_n
    dsr = np.where((s >= 0.0) & (s <= 1.0), np.sign(d) * inv_n, 0.0)
    return np.array([loss]), np.array([mag]), dsr


def c_flat_sum(n):
    """The constant of ff_l1_loss_grad's loss and ff_grad_sqnorm, DERIVED from the kernels' fixed order (l1_stage1_kernel /
    sqnorm_stage1_kernel + sum_finish_kernel): every level of additions costs at most 2^-24 * sum |terms|.  nb = min(1024, ceil(n / 256))
    workgroups; a thread adds ceil(n / (256 nb)) terms one after the other, an 8-level tree follows, the finish adds ceil(nb / 256)
    partials per thread and runs another 8-level tree; 2 for the term itself (the difference or the square, and |.|'s operand), 1 for
    the final scale.  A strictly sequential sum of 262147 positive terms is far worse (measured ~1000), so it is no model here."""
    nb = min(1024, -(-n // 256))
    return -(-n // (256 * nb)) + 8 + -(-nb // 256) + 8 + 3


def sqnorm_ref(g):
    g = f64(g)
    v = (g * g).sum()
    return np.array([v]), np.array([v])


# ---------------------------------------------------------------------------------------------------------------------
# exact data movement
PERMUTE_CASES = [(5, 7, 1), (9, 30, 3), (30, 9, 65)]             # (A, Bd, C): [A][Bd][C] -> [Bd][A][C]
TAPS_CASES = [(9, 1), (21, 3), (25, 65)]                         # (taps, C)
FLIPT_CASES = [(3, 1, 3, 3), (65, 3, 1, 3), (4, 65, 5, 5), (1, 3, 3, 1)]     # (Cout, Cin, KH, KW)


def permute_rows_ref(x, A, Bd, C):
    return np.ascontiguousarray(x.reshape(A, Bd, C).transpose(1, 0, 2))


def taps_reverse_ref(w):
    return np.ascontiguousarray(w[::-1])


def conv_weight_flipT_ref(w, Cout, Cin, taps):
    """wt[ci][taps - 1 - t][co] = w[co][t][ci]."""
    return np.ascontiguousarray(w.reshape(Cout, taps, Cin)[:, ::-1].transpose(2, 1, 0))


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm2d in training mode, one module call per group of rows (the tape's batchnorm_train and ff_bn_*)
# C_BN_BWD is measured like the other reduction constants, on a stand-in of the tape's sequence: column sums, mean = s1 * fp32(1 / n),
# xc = x - mean, column sums of xc^2, ff_bn_train_finish, y = x scale + shift; backward with ff_bn_xhat and two more column sums.
# Conditioning as for LayerNorm: x - mean is off by a multiple of 2^-24 xm, xm = |x| + |mean|; rstd by the relative
# kappa = mean(|x - mean| xm) / (var + eps) >= 1 (80 for x = 5 + 0.1 noise); xhat carries xhm = xm rstd + |xhat| kappa.
# C_BN_STAT holds the forward and the running statistics (a sequential sum of 513 values near 5 is what makes it large),
# C_BN_BWD the three gradients.
C_BN_STAT_MEASURED = 14.8
C_BN_BWD_MEASURED = 5.9
C_BN_STAT = REDUCTION_FACTOR * C_BN_STAT_MEASURED
C_BN_BWD = REDUCTION_FACTOR * C_BN_BWD_MEASURED
BN_CONST = dict(y="C_BN_STAT", running_mean="C_BN_STAT", running_var="C_BN_STAT", dx="C_BN_BWD", dgamma="C_BN_BWD", dbeta="C_BN_BWD",
                xhat="C_BN_BWD")
BN_CASES = [(G, C, rpg) for G in (1, 3, 9) for C in (3, 64, 65) for rpg in (7, 513)]
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def bn_inputs(case, seed=0):
    G, C, rpg = case
    return dict(x=draw(seed + 1, G * rpg, C, scale=0.1, shift=5.0), gamma=draw(seed + 2, C, scale=0.2, shift=1.0), beta=draw(seed + 3, C, scale=0.1),
                dy=draw(seed + 4, G * rpg, C), rm0=draw(seed + 5, C, scale=0.1), rv0=np.abs(draw(seed + 6, C)) + np.float32(0.5))


def batchnorm_train_ref(x, gamma, beta, rm0, rv0, dy, G, eps=BN_EPS, momentum=BN_MOMENTUM):
    """-> dict name -> (ref, mag): y, running_mean, running_var, dx, dgamma, dbeta, xhat, and mean_rstd / sdy / sdyxh (refs only)."""
    C = x.shape[-1]
    x, dy, gamma, beta = f64(x).reshape(G, -1, C), f64(dy).reshape(G, -1, C), f64(gamma), f64(beta)
    n = x.shape[1]
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    mean = x.mean(1, keepdims=True)
    d = x - mean
    var = (d * d).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xm = np.abs(x) + np.abs(mean)
    kappa = np.maximum((np.abs(d) * xm).mean(1, keepdims=True) / (var + eps), 1.0)
    sc = gamma * rstd
    y, y_mag = d * sc + beta, np.abs(sc) * (xm + kappa * np.abs(d)) + np.abs(beta)
    rm, rmm, rv, rvm = f64(rm0), np.abs(f64(rm0)), f64(rv0), np.abs(f64(rv0))
    for g in range(G):
        vu = var[g, 0] * (n / (n - 1.0) if n > 1 else 1.0)
        rm, rmm = (1 - momentum) * rm + momentum * mean[g, 0], (1 - momentum) * rmm + momentum * np.abs(x[g]).mean(0)
        rv, rvm = (1 - momentum) * rv + momentum * vu, (1 - momentum) * rvm + momentum * vu * kappa[g, 0]
    xh = d * rstd
    xha, xhm = np.abs(xh), xm * rstd + np.abs(xh) * kappa
    sdy, sdyxh = dy.sum(1, keepdims=True), (dy * xh).sum(1, keepdims=True)
    dx = sc * (dy - sdy / n - xh * sdyxh / n)
    dya = np.abs(dy)
    dx_mag = np.abs(sc) * (dya + dya.mean(1, keepdims=True) + xha * (dya * xha).mean(1, keepdims=True) + xhm * np.abs(sdyxh / n)
                           + xha * (dya * xhm).mean(1, keepdims=True)) + kappa * np.abs(dx)
    flat = lambda a: a.reshape(-1, C)
    return dict(y=(flat(y), flat(y_mag)), running_mean=(rm, rmm), running_var=(rv, rvm), dx=(flat(dx), flat(dx_mag)),
                dgamma=(sdyxh.sum((0, 1)), (dya * xhm).sum((0, 1))), dbeta=(sdy.sum((0, 1)), dya.sum((0, 1))), xhat=(flat(xh), flat(xhm)),
                mean_rstd=np.stack([mean[:, 0], rstd[:, 0]], -1), sdy=sdy[:, 0], sdyxh=sdyxh[:, 0])


# ---------------------------------------------------------------------------------------------------------------------
# adjoint of F.interpolate(bilinear, align_corners=False)
# The kernel evaluates the forward's source coordinate s = max(sc (o + 0.5) - 0.5, 0) in fp32 (error up to 2 * 2^-24 (s + 1)), so a tap
# weight is uncertain by that much, and next to an integer s the fp32 floor may pick the neighbouring pair of taps: the mag of an
# input pixel therefore carries (s + 1) |dy| for every output whose taps, or their direct neighbours, touch it.  C_RESIZE_ADJ is
# measured on an fp32 stand-in of the kernel's gather (sequential over ox, then over oy) like the reduction constants.
C_RESIZE_ADJ_MEASURED = 0.73
C_RESIZE_ADJ = REDUCTION_FACTOR * C_RESIZE_ADJ_MEASURED
RESIZE_CASES = [(1, 1, 7, 5, None), (7, 5, 1, 1, None), (3, 4, 64, 33, None), (33, 64, 4, 3, None), (10, 10, 3, 3, 0.3)]     # Hi, Wi, Ho, Wo, sf
RESIZE_MUL = 0.5


def aten_scale(n_in, n_out, sf, dtype=np.float32):
    """ATen's area_pixel_compute_scale (align_corners=False): 1 / scale_factor if given, else in / out."""
    return float(dtype(1.0) / dtype(sf)) if sf else float(dtype(n_in) / dtype(n_out))


def resize_axis(n_in, n_out, sc, dtype=np.float64):
    """-> A [n_in, n_out], the forward's tap weights evaluated in `dtype`, and E, the (s + 1) uncertainty where a tap may fall."""
    A, E = np.zeros((n_in, n_out), dtype), np.zeros((n_in, n_out))
    if n_in == n_out:
        return np.eye(n_in, dtype=dtype), E
    for o in range(n_out):
        s = max(dtype(sc) * (dtype(o) + dtype(0.5)) - dtype(0.5), dtype(0))
        i0 = min(int(np.floor(s)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        lam = min(max(s - dtype(i0), dtype(0)), dtype(1))
        A[i0, o] += dtype(1) - lam
        A[i1, o] += lam
        E[max(i0 - 1, 0):min(i1 + 1, n_in - 1) + 1, o] = float(s) + 1.0
    return A, E


def resize_adj_ref(dy, Hi, Wi, sh, sw, mul, dx0=None):
    """dy [B, Ho, Wo, C] -> dx [B, Hi, Wi, C] = mul * Ay dy Ax^T (+ dx0)."""
    dy = f64(dy)
    Ay, Ey = resize_axis(Hi, dy.shape[1], sh)
    Ax, Ex = resize_axis(Wi, dy.shape[2], sw)
    app = lambda P, Q, t: np.einsum("yo,bopc,xp->byxc", P, t, Q)
    ref = mul * app(Ay, Ax, dy)
    mag = abs(mul) * (app(Ay, Ax, np.abs(dy)) + app(Ey, Ax, np.abs(dy)) + app(Ay, Ex, np.abs(dy)))
    if dx0 is not None:
        ref, mag = ref + f64(dx0), mag + np.abs(f64(dx0))
    return ref, mag


# ---------------------------------------------------------------------------------------------------------------------
# one clip + AdamW + EMA step over a flat buffer (ff_adamw_ema_step).  hyper: lr, beta1, beta2, eps, weight_decay, max_norm, ema_decay,
# step, step_size = lr / (1 - beta1^step), sqrt(1 - beta2^step).
# C_ADAMW = 16 is an upper count of the roundings of adamw_ema_kernel, each taken on the mag of the term it touches:
#   coef   sqrtf, + 1e-6, the division: 3;  g' = g coef: 4 on |g'|
#   m'     g' - m 1, 1 - beta1 1, the product 1, the sum 1, on top of g's 4: 8 on |m| + (|g'| + |m|) (1 - beta1)
#   v'     v beta2 1; 1 - beta2 1, times g' twice 2 + 2 * 4, the sum 1: 13 on |v beta2| + (1 - beta2) g'^2
#   p'     denom = sqrtf(v') / bc2s + eps: 13 / 2 + 3; m' / denom 1, step_size 1, p (1 - lr wd) 3, the difference 1:
#          at most 13 on |p| + step_size (|m|-mag + |m'|) / denom
#   ema'   decay ema 1, 1 - decay 1, times p' 1, the sum 1, on top of p's 13: 16 on |decay ema| + (1 - decay) p-mag
C_ADAMW = 16.0
ADAMW_HYPER = dict(lr=1.5e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4, decay=0.9995, step=3)


def adamw_hyper(max_norm, dtype=np.float32):
    h = ADAMW_HYPER
    v = [h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], max_norm, h["decay"], h["step"], h["lr"] / (1 - h["b1"] ** h["step"]),
         math.sqrt(1 - h["b2"] ** h["step"])]
    return np.array(v, dtype=dtype)


def adamw_inputs(n, seed=0):
    return dict(p=draw(seed + 1, n), g=draw(seed + 2, n, scale=0.01), m=draw(seed + 3, n, scale=0.01),
                v=(draw(seed + 4, n, scale=0.01) ** 2).astype(np.float32), ema=draw(seed + 5, n))


def adamw_ema_ref(p, g, m, v, ema, hyper, sqnorm):
    """-> dict name -> (ref, mag) for g, m, v, p, ema after the step; hyper as the kernel reads it (10 values), sqnorm = sum g^2."""
    p, g, m, v, hy = f64(p), f64(g), f64(m), f64(v), f64(hyper)
    lr, b1, b2, eps, wd, max_norm, decay, _, step_size, bc2s = hy
    coef = min(max_norm / (math.sqrt(float(sqnorm)) + float(np.float32(1e-6))), 1.0) if max_norm > 0 else 1.0
    gi = g * coef
    mi, mm = m + (gi - m) * (1 - b1), np.abs(m) + (np.abs(gi) + np.abs(m)) * abs(1 - b1)
    vi = v * b2 + (1 - b2) * gi * gi
    denom = np.sqrt(vi) / bc2s + eps
    pi = p * (1 - lr * wd) - step_size * (mi / denom)
    pm = np.abs(p) + step_size * (mm + np.abs(mi)) / denom
    out = dict(g=(gi, np.abs(gi)), m=(mi, mm), v=(vi, vi), p=(pi, pm))
    if ema is not None:
        e = f64(ema)
        out["ema"] = (decay * e + (1 - decay) * pi, np.abs(decay * e) + abs(1 - decay) * pm)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rfft2 / irfft2 (norm = 'ortho') as the two direct DFT passes of csrc/freq.hip, over SPEC_CASES x SPEC_PLANES.
# mag of a second-pass output: the absolute values of its own terms plus twice the mag of the first pass's outputs it reads (both
# components of each), since those arrive with their own error.  C_DFT is measured on an fp32 stand-in (fp32 twiddle tables,
# strictly sequential sums) like the other reduction constants.
C_DFT_MEASURED = 0.62
C_DFT = REDUCTION_FACTOR * C_DFT_MEASURED


def rfft2_ref(x):
    """x [C, H, W] -> spec, mag [C, H, Wf, 2]."""
    x = f64(x)
    H, W = x.shape[1:]
    Y = np.fft.rfft(x, axis=2, norm="ortho")
    m1 = np.abs(x).sum(2, keepdims=True) / math.sqrt(W)
    Z = np.fft.fft(Y, axis=1, norm="ortho")
    mag = ((np.abs(Y.real) + np.abs(Y.imag)).sum(1, keepdims=True) + 2.0 * m1.sum(1, keepdims=True)) / math.sqrt(H)
    ref = np.stack([Z.real, Z.imag], -1)
    return ref, np.broadcast_to(mag[..., None], ref.shape).copy()


def irfft2_ref(spec, W):
    """spec [C, H, Wf, 2] -> planes, mag [C, H, W]; the imaginary parts of the DC and (even W) Nyquist columns are ignored, as torch's
    c2r transform does."""
    spec = f64(spec)
    H, Wf = spec.shape[1:3]
    S = spec[..., 0] + 1j * spec[..., 1]
    U = np.fft.ifft(S, axis=1, norm="ortho")
    mU = (np.abs(spec[..., 0]) + np.abs(spec[..., 1])).sum(1, keepdims=True) / math.sqrt(H)         # [C, 1, Wf]
    out = np.fft.irfft(U, n=W, axis=2, norm="ortho")
    k = np.arange(Wf)
    single = (k == 0) | ((W % 2 == 0) & (k == W // 2))
    f = np.where(single, 1.0, 2.0)
    own = np.abs(U.real) + np.where(single, 0.0, np.abs(U.imag))
    mag = ((f * own).sum(2, keepdims=True) + 2.0 * (f * mU).sum(2, keepdims=True)) / math.sqrt(W)   # [C, H, 1]
    return out, np.broadcast_to(mag, out.shape).copy()


# ---------------------------------------------------------------------------------------------------------------------
# ff_bn_train_finish on its own, from given column sums: s2 = sum (x - mean)^2 (centered) or sum x^2 (then var = s2 / n - mean^2, whose
# cancellation kappa = (s2 / n + mean^2) / (var + eps) multiplies whatever carries rstd or the variance).
# C_BN_FINISH = 12, an upper count of bn_train_finish_kernel's roundings: var 5 kappa (s2 / n 1, mean^2 3, the difference 1), + eps 1,
# sqrtf and the division 2 on half of that: rstd 6 kappa; scale 1 more, shift 3 more; the running variance 5 kappa + 6 per group.
C_BN_FINISH = 12.0
BN_FINISH_CASES = [(G, C, n, shift, scale) for G in (1, 3) for C in (3, 65, 300) for n, shift, scale in ((1, 0.7, 1.5), (7, 0.7, 1.5), (513, 5.0, 0.1))]


def bn_finish_inputs(case, centered, seed=0):
    """Column sums of seeded data, rounded to fp32 as a kernel would hand them over."""
    G, C, n, shift, scale = case
    x = f64(draw(seed + 1, G, n, C, scale=scale, shift=shift))
    s1 = x.sum(1)
    s2 = ((x - s1[:, None] / n) ** 2).sum(1) if centered else (x * x).sum(1)
    return dict(s1=s1.astype(np.float32), s2=s2.astype(np.float32), gamma=draw(seed + 2, C, scale=0.2, shift=1.0), beta=draw(seed + 3, C, scale=0.1),
                rm0=draw(seed + 5, C, scale=0.1), rv0=np.abs(draw(seed + 6, C)) + np.float32(0.5))


def bn_finish_ref(s1, s2, centered, n, gamma, beta, rm0, rv0, eps=BN_EPS, momentum=BN_MOMENTUM):
    """-> dict name -> (ref, mag): mean_rstd [G, C, 2], scale, shift [G, C], running_mean, running_var [C]."""
    s1, s2, gamma, beta = f64(s1), f64(s2), f64(gamma), f64(beta)
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    mean = s1 / n
    var = np.maximum(s2 / n if centered else s2 / n - mean * mean, 0.0)
    kappa = np.ones_like(var) if centered else np.maximum((s2 / n + mean * mean) / (var + eps), 1.0)
    rstd = 1.0 / np.sqrt(var + eps)
    sc = gamma * rstd
    out = dict(mean_rstd=(np.stack([mean, rstd], -1), np.stack([np.abs(mean), rstd * kappa], -1)), scale=(sc, np.abs(sc) * kappa),
               shift=(beta - mean * sc, np.abs(beta) + np.abs(mean * sc) * kappa))
    rm, rmm, rv, rvm = f64(rm0), np.abs(f64(rm0)), f64(rv0), np.abs(f64(rv0))
    for g in range(s1.shape[0]):
        vu = var[g] * (n / (n - 1.0) if n > 1 else 1.0)
        rm, rmm = (1 - momentum) * rm + momentum * mean[g], (1 - momentum) * rmm + momentum * np.abs(mean[g])
        rv, rvm = (1 - momentum) * rv + momentum * vu, (1 - momentum) * rvm + momentum * (vu + (s2[g] / n + mean[g] ** 2) * (0 if centered else 1))
    out.update(running_mean=(rm, rmm), running_var=(rv, rvm))
    return out
