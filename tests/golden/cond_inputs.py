"""Ill-conditioned input families, fp64 references and fp32 stand-ins for the fp32-grade ('bf16x3' / 'f32') kernels (pure torch, CPU).

The op-level GPU tests draw zero-mean, unit-scale rows and compare one max-abs error with the global max|ref|: the one input family on
which LayerNorm, softmax and the activation tails cannot go wrong.  This module supplies the rows a network produces instead.

LayerNorm rows (ln_rows): one [M, C] tensor of contiguous, named blocks -- FAMILIES below.  M is chosen by the caller so that the last
32-row tile is ragged (77, 109, 153).

Attention inputs (attn_qkv): four families whose answers do not depend on the precision of the logits -- `uniform` (q = 0: the logits
are the bias alone), `onehot` (one key per window wins every query by a logit gap >= 40), `tie` (two identical keys share the maximum),
`masked` (q = 0, zero bias, shifted windows: the -100 mask leaves the keys of the query's own region, the output is their mean v).
attn_proj_case builds the same families through a qkv projection (win_attn_fused), ocab_qkv for overlapping key windows (ocab_attn).

The rule every comparison follows (family_errors / allowance / check):
  * a chain is a function of a dtype: evaluated in torch.float64 it is the reference, in torch.float32 (two-pass LayerNorm, the form
    of stage_ref.layernorm_fp32) it is the stand-in -- what plain fp32 arithmetic achieves on these very tensors;
  * errors are normalised per family, by max(1, max|ref|) over that family's rows, never over the whole tensor (the `huge` and
    `spike` blocks would hide everything else);
  * an op's allowance on a family is its existing bar in tests/test_ops_gpu.py plus FACTOR = 4 times the stand-in's own error on
    that family, computed at run time from the same tensors; the factor covers the kernels' different but fixed summation order
    (lane-pair halves, st-major).
tests/test_cond_inputs_cpu.py checks the families' properties and the stand-ins; tests/test_conditioning_gpu.py holds the kernels."""
import math

import torch
import torch.nn.functional as F

FACTOR = 4.0
STANDIN_CAP = 1e-4          # a family whose fp32 stand-in is further than this from fp64 is outside what fp32 can do
F64, F32 = torch.float64, torch.float32

# name -> (kind, mean, sigma); the nominal mean / std that test_cond_inputs_cpu.py checks
FAMILIES = [
    ("control", ("randn", 0.0, 1.0)),
    ("offset_8_1", ("randn", 8.0, 1.0)),
    ("offset_64_1", ("randn", 64.0, 1.0)),
    ("offset_1000_1", ("randn", 1000.0, 1.0)),
    ("offset_m300_0.5", ("randn", -300.0, 0.5)),
    ("lowvar_0", ("randn", 0.0, 1e-3)),
    # `lowvar` at m = 5 is left out: fp32 cannot do it.  The row mean carries a rounding of ~3e-7 (half an ulp of 5) against a spread of
    # 1e-3, so the two-pass fp32 stand-in of a bare LayerNorm is already 1.0e-4 (C = 180, 1024) to 2.8e-4 (C = 64) from fp64, over STANDIN_CAP.
    ("const_3", ("const", 3.0, 0.0)),
    ("const_0.1", ("const", 0.1, 0.0)),
    ("spike", ("spike", 1e4, 0.0)),
    ("tiny", ("randn", 0.0, 1e-4)),
    ("huge", ("randn", 0.0, 1e4)),
]
OFFSET_FAMILIES = [n for n, _ in FAMILIES if n.startswith("offset")]


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def ln_rows(M: int, C: int, seed: int = 0, skip=()):
    """-> (x [M, C] fp32, fam: dict name -> slice of rows).  Every family gets M // n rows, `control` the remainder as well."""
    fams = [(n, s) for n, s in FAMILIES if n not in skip]
    per = M // len(fams)
    assert per >= 2, "too few rows for the families"
    blocks, fam, r0 = [], {}, 0
    for i, (name, (kind, m, s)) in enumerate(fams):
        rows = per + (M - per * len(fams) if i == 0 else 0)
        if kind == "randn":
            b = (m + s * rnd(rows, C, seed=seed * 100 + i).double()).float()
        elif kind == "const":
            b = torch.full((rows, C), m, dtype=F32)
        else:
            b = torch.zeros(rows, C)
            b[torch.arange(rows), (torch.arange(rows) * 37 + 5) % C] = m
        blocks.append(b)
        fam[name] = slice(r0, r0 + rows)
        r0 += rows
    return torch.cat(blocks).contiguous(), fam


def ln_params(C: int, seed: int):
    return rnd(C, seed=seed) * 0.1 + 1, rnd(C, seed=seed + 1) * 0.1


def lin_params(n: int, k: int, seed: int):
    return rnd(n, k, seed=seed, scale=1.0 / math.sqrt(k)), rnd(n, seed=seed + 1, scale=0.1)


# ------------------------------------------------------------------------------------------------------------------------------
# chains: every function takes fp32 tensors and a dtype and evaluates in that dtype (fp64: reference, fp32: stand-in)
def layernorm(x, g, b, eps, dt):
    """Two-pass LayerNorm in dt (stage_ref.layernorm_fp32's form)."""
    x, g, b = x.to(dt), g.to(dt), b.to(dt)
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(-1, keepdim=True) / C + eps)
    return d * rstd * g + b


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))


def linear(x, w, b, dt):
    return F.linear(x.to(dt), w.to(dt), None if b is None else b.to(dt))


def token_linear(x, g, b, eps, w, bias, act, dt):
    """-> (act(LayerNorm(x) W^T + bias), LayerNorm(x))"""
    xn = layernorm(x, g, b, eps, dt)
    y = linear(xn, w, bias, dt)
    return (gelu(y) if act == "gelu" else y), xn


def token_mlp(x, g, b, w1, b1, w2, b2, dt, eps=1e-5):
    return x.to(dt) + linear(gelu(linear(layernorm(x, g, b, eps, dt), w1, b1, dt)), w2, b2, dt)


def token_projmlp(att, x, wp, bp, w1, b1, w2, b2, g, b, dt, eps=1e-5):
    x1 = x.to(dt) + linear(att, wp, bp, dt)
    return x1 + linear(gelu(linear(layernorm(x1, g, b, eps, dt), w1, b1, dt)), w2, b2, dt)


def naf_ffn(y, g, b, w4, b4, w5, b5, gam, dt, eps=1e-6):
    C = y.shape[-1]
    t = linear(layernorm(y, g, b, eps, dt), w4, b4, dt)
    return y.to(dt) + gam.to(dt) * linear(t[:, :C] * t[:, C:], w5, b5, dt)


def dw3x3(t, wd, bd, dt):
    """Depth-wise 3x3 with zero padding as nine shifted products (no fp64 convolution backend needed).  t [H, W, C], wd [C, 1, 3, 3]."""
    H, W, C = t.shape
    tp = F.pad(t.to(dt), (0, 0, 1, 1, 1, 1))
    out = torch.zeros(H, W, C, dtype=dt) + (0 if bd is None else bd.to(dt))
    for ky in range(3):
        for kx in range(3):
            out = out + tp[ky:ky + H, kx:kx + W] * wd[:, 0, ky, kx].to(dt)
    return out


def naf_front(x, g, b, w1, b1, w2, b2, dt, eps=1e-6):
    """x [H, W, C] -> (SimpleGate(dw3x3(conv1(LayerNorm2d(x)))) [H, W, C], its mean over the pixels [C])"""
    H, W, C = x.shape
    t = linear(layernorm(x.reshape(H * W, C), g, b, eps, dt), w1, b1, dt).reshape(H, W, 2 * C)
    t = dw3x3(t, w2, b2, dt)
    out = t[..., :C] * t[..., C:]
    return out, out.mean(dim=(0, 1))


def spatial_gate(y, H, W, g2, b2, wd, bd, dt, eps=1e-5):
    """DAT SpatialGate on an fc1 output y [H*W, 2c]: y[:, :c] * (dw3x3(LayerNorm(y[:, c:])) + bd)"""
    c = y.shape[-1] // 2
    xn = layernorm(y[:, c:], g2, b2, eps, dt).reshape(H, W, c)
    return y[:, :c].to(dt).reshape(H, W, c) * dw3x3(xn, wd, bd, dt)


def hat_attn(x, g, b, wqkv, bqkv, table, heads, d, win, shift, dt, eps=1e-5):
    """HAB attention half on x [1, H, W, C]: norm1, qkv, (S)W-MSA -> (normalised rows [H*W, C], attention output [H*W, C])"""
    _, H, W, C = x.shape
    xn = layernorm(x.reshape(H * W, C), g, b, eps, dt)
    qkv = linear(xn, wqkv, bqkv, dt).reshape(1, H, W, 3 * C)
    return xn, window_attention(qkv, table, heads, d, win, shift, dt).reshape(H * W, C)


def chan_qkv(x, g, b, wqkv, bqkv, temp, heads, dt, eps=1e-5):
    """-> (v [M, C], block-diagonal channel attention matrix [C, C])"""
    M, C = x.shape
    d = C // heads
    qkv = linear(layernorm(x, g, b, eps, dt), wqkv, bqkv, dt)
    q = qkv[:, :C].reshape(M, heads, d).permute(1, 2, 0)
    k = qkv[:, C:2 * C].reshape(M, heads, d).permute(1, 2, 0)
    a = torch.softmax((F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)) * temp.to(dt)[:, None, None], dim=-1)
    return qkv[:, 2 * C:], torch.block_diag(*[a[h] for h in range(heads)])


# ------------------------------------------------------------------------------------------------------------------------------
# window attention
def win_split(x, wh, ww):
    b, h, w, c = x.shape
    return x.reshape(b, h // wh, wh, w // ww, ww, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, wh * ww, c)


def win_merge(x, wh, ww, h, w):
    c = x.shape[-1]
    b = x.shape[0] // ((h // wh) * (w // ww))
    return x.reshape(b, h // wh, w // ww, wh, ww, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)


def region_labels(h, w, wh, ww, sh, sw):
    lab = torch.zeros(h, w)
    cnt = 0
    for hs in (slice(0, -wh), slice(-wh, -sh), slice(-sh, None)):
        for ws in (slice(0, -ww), slice(-ww, -sw), slice(-sw, None)):
            lab[hs, ws] = cnt
            cnt += 1
    return win_split(lab.reshape(1, h, w, 1), wh, ww).squeeze(-1)            # (nwin, n), in the rolled frame


def rel_index(wh, ww):
    cy, cx = torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="ij")
    cy, cx = cy.reshape(-1), cx.reshape(-1)
    return (cy[:, None] - cy[None, :] + wh - 1) * (2 * ww - 1) + (cx[:, None] - cx[None, :] + ww - 1)


def window_attention(qkv, table, heads, d, win, shift, dt, scale=None):
    """qkv [1, H, W, 3 heads d] -> [1, H, W, heads d]: (shifted-)window attention with the relative-position bias table [heads, (2wh-1)(2ww-1)]
    and the -100 region mask when shift != (0, 0); softmax in dt."""
    wh, ww = win
    _, H, W, _ = qkv.shape
    C = heads * d
    scale = d ** -0.5 if scale is None else scale
    bias = table.to(dt)[:, rel_index(wh, ww)]                                # (heads, nq, nk)
    xi = qkv.to(dt)
    shifted = shift[0] > 0 or shift[1] > 0
    if shifted:
        xi = torch.roll(xi, shifts=(-shift[0], -shift[1]), dims=(1, 2))
    xw = win_split(xi, wh, ww).reshape(-1, wh * ww, 3, heads, d).permute(2, 0, 3, 1, 4)
    a = (xw[0] * scale) @ xw[1].transpose(-2, -1) + bias.unsqueeze(0)
    if shifted:
        lab = region_labels(H, W, wh, ww, shift[0], shift[1])
        a = a + torch.where(lab.unsqueeze(1) != lab.unsqueeze(2), -100.0, 0.0).to(dt)[:, None]
    o = (torch.softmax(a, dim=-1) @ xw[2]).transpose(1, 2).reshape(-1, wh * ww, C)
    o = win_merge(o, wh, ww, H, W)
    return torch.roll(o, shifts=shift, dims=(1, 2)) if shifted else o


ATTN_FAMILIES = ("uniform", "onehot", "tie", "masked")
ONEHOT_LOGIT = 26.0         # scale * |q||k| of the winning key; every other key sits at <= -0.6 of it: gap >= 41.6


def attn_tokens(family, n_windows, n, heads, d, seed, scale=None, logit=ONEHOT_LOGIT, u_global=False, winners=None):
    """q, k, v [n_windows, n, heads, d] for one family (window-major; `masked` is `uniform` under a shift).  -> (q, k, v, info);
    info["winner"] / info["second"]: the winning key indices per (window, head) of `onehot` / `tie`.  logit: scale * |q||k| of the
    winning key; u_global: one key direction per head for every window (overlapping key windows); winners: where a winner may sit."""
    scale = d ** -0.5 if scale is None else scale
    v = rnd(n_windows, n, heads, d, seed=seed)
    if family in ("uniform", "masked"):
        return torch.zeros(n_windows, n, heads, d), rnd(n_windows, n, heads, d, seed=seed + 1), v, {}
    g = torch.Generator(device="cpu").manual_seed(seed + 2)
    u = F.normalize(torch.randn(1 if u_global else n_windows, 1, heads, d, generator=g), dim=-1).expand(n_windows, 1, heads, d)
    A = math.sqrt(logit / scale)
    r = 0.6 + 0.4 * torch.rand(n_windows, n, heads, 1, generator=g)
    t = 1.0 + 0.2 * torch.rand(n_windows, n, heads, 1, generator=g)
    k = -r * A * u
    q = (t * A * u).expand(n_windows, n, heads, d).contiguous()
    if winners is None:
        win = torch.randint(0, n, (n_windows, heads), generator=g)
        sec = (win + 1 + torch.randint(0, n - 1, (n_windows, heads), generator=g)) % n
    else:                                               # winners: the token indices a winner may take (at least two)
        cand = torch.as_tensor(winners)
        pick = torch.randint(0, len(cand), (n_windows, heads), generator=g)
        win = cand[pick]
        sec = cand[(pick + 1 + torch.randint(0, len(cand) - 1, (n_windows, heads), generator=g)) % len(cand)]
    wi, hi = torch.meshgrid(torch.arange(n_windows), torch.arange(heads), indexing="ij")
    k[wi, win, hi] = (A * u[:, 0])
    if family == "tie":
        k[wi, sec, hi] = k[wi, win, hi]
    return q, k.contiguous(), v, {"winner": win, "second": sec}


def attn_exact(family, q, k, v, info):
    """The precision-independent answer of onehot / tie, [n_windows, n, heads, d] (every query of a window gets the same row)."""
    nw, n, heads, d = v.shape
    wi, hi = torch.meshgrid(torch.arange(nw), torch.arange(heads), indexing="ij")
    row = v.double()[wi, info["winner"], hi]
    if family == "tie":
        row = 0.5 * (row + v.double()[wi, info["second"], hi])
    return row[:, None].expand(nw, n, heads, d)


def attn_qkv(family, H, W, heads, d, win, seed):
    """qkv [1, H, W, 3 heads d] for window_attention(shift = (wh/2, ww/2) for `masked`, else none) -> (qkv, info)."""
    wh, ww = win
    nw = (H // wh) * (W // ww)
    q, k, v, info = attn_tokens(family, nw, wh * ww, heads, d, seed)
    qkv = torch.cat([win_merge(t.reshape(nw, wh * ww, heads * d), wh, ww, H, W) for t in (q, k, v)], dim=-1)
    if family == "masked":                                                   # the windows are cut in the rolled frame
        qkv = torch.roll(qkv, shifts=(wh // 2, ww // 2), dims=(1, 2))
    return qkv.contiguous(), info


def attn_proj_case(family, H, W, win, heads, d, seed):
    """The attention families THROUGH a qkv projection (win_attn_fused; no LayerNorm: gamma = None): -> (x [1, H, W, C], wqkv [3C, C],
    bqkv [3C], info).  Channel 0 of a token is its query strength t (0 for `uniform` / `masked`: q = 0 exactly, the q weights are zero
    elsewhere and the q bias is zero), channel 1 + h its key coefficient for head h (+1 for the winner, -r otherwise), the rest randn;
    q_h = t A u_h, k_h = coefficient A u_h, v = a random projection of the whole token.  The logits of `onehot` / `tie` are
    ONEHOT_LOGIT t coefficient: the gap is >= 41.6 and a projection error of 2^-16 of them does not touch it; identical coefficients give
    bit-identical keys.  The exact answer is the projected v row of the winner (proj_attention in fp64)."""
    wh, ww = win
    C, n, nw = heads * d, wh * ww, (H // wh) * (W // ww)
    g = torch.Generator(device="cpu").manual_seed(seed)
    xw = torch.randn(nw, n, C, generator=g)
    info = {}
    if family in ("uniform", "masked"):
        xw[:, :, 0] = 0.0
    else:
        xw[:, :, 0] = 1.0 + 0.2 * torch.rand(nw, n, generator=g)
        xw[:, :, 1:1 + heads] = -(0.6 + 0.4 * torch.rand(nw, n, heads, generator=g))
        winr = torch.randint(0, n, (nw, heads), generator=g)
        sec = (winr + 1 + torch.randint(0, n - 1, (nw, heads), generator=g)) % n
        wi, hi = torch.meshgrid(torch.arange(nw), torch.arange(heads), indexing="ij")
        xw[wi, winr, 1 + hi] = 1.0
        if family == "tie":
            xw[wi, sec, 1 + hi] = 1.0
        info = {"winner": winr, "second": sec}
    x = win_merge(xw, wh, ww, H, W)
    if family == "masked":
        x = torch.roll(x, shifts=(wh // 2, ww // 2), dims=(1, 2))
    u = F.normalize(torch.randn(heads, d, generator=g), dim=-1)
    A = math.sqrt(ONEHOT_LOGIT / d ** -0.5)
    w = torch.zeros(3 * C, C)
    for h in range(heads):
        w[h * d:(h + 1) * d, 0] = A * u[h]
        w[C + h * d:C + (h + 1) * d, 1 + h] = A * u[h]
    w[2 * C:] = torch.randn(C, C, generator=g) / math.sqrt(C)
    b = torch.zeros(3 * C)
    b[2 * C:] = 0.1 * torch.randn(C, generator=g)
    return x.contiguous(), w, b, info


def proj_attention(x, wqkv, bqkv, table, heads, d, win, shift, dt):
    """-> (window attention of the projected rows [1, H, W, C], the projected v [1, H, W, C])"""
    _, H, W, C = x.shape
    qkv = linear(x.reshape(H * W, C), wqkv, bqkv, dt).reshape(1, H, W, 3 * C)
    return window_attention(qkv, table, heads, d, win, shift, dt), qkv[..., 2 * C:]


def ocab_rel_index(ws, ows):
    """hat_arch.py's overlapping-window index: its offset ws - ows + 1 is negative, the gather wraps."""
    ys, xs = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    ye, xe = torch.meshgrid(torch.arange(ows), torch.arange(ows), indexing="ij")
    dy = ye.reshape(-1)[None, :] - ys.reshape(-1)[:, None] + ws - ows + 1
    dx = xe.reshape(-1)[None, :] - xs.reshape(-1)[:, None] + ws - ows + 1
    return dy * (ws + ows - 1) + dx


def ocab_attention(qkv, table, heads, d, ws, ows, dt):
    """HAT OCAB: ws x ws query windows against ows x ows key windows cut with zero padding (the zero keys enter the softmax at their
    bias); table [(ws+ows-1)^2, heads].  qkv [1, H, W, 3C] -> [1, H, W, C]"""
    _, H, W, _ = qkv.shape
    C, nw = heads * d, (H // ws) * (W // ws)
    qkv = qkv.to(dt)
    n = (ws + ows - 1) ** 2
    bias = table.to(dt)[ocab_rel_index(ws, ows).reshape(-1) % n].reshape(ws * ws, ows * ows, heads).permute(2, 0, 1)
    q = win_split(qkv[..., :C], ws, ws)
    kvw = F.unfold(qkv[..., C:].permute(0, 3, 1, 2), kernel_size=ows, stride=ws, padding=(ows - ws) // 2)
    kvw = kvw.reshape(1, 2, C, ows * ows, nw).permute(1, 0, 4, 3, 2).reshape(2, nw, ows * ows, C)
    qh = q.reshape(-1, ws * ws, heads, d).transpose(1, 2) * d ** -0.5
    kh = kvw[0].reshape(-1, ows * ows, heads, d).transpose(1, 2)
    vh = kvw[1].reshape(-1, ows * ows, heads, d).transpose(1, 2)
    a = torch.softmax(qh @ kh.transpose(-2, -1) + bias.unsqueeze(0), dim=-1)
    return win_merge((a @ vh).transpose(1, 2).reshape(-1, ws * ws, C), ws, ws, H, W)


OCAB_LOGIT = 44.0           # the zero-padded keys of an overlapping window sit at logit 0: the winner needs its 40 against them too


def ocab_qkv(family, H, W, heads, d, ws, seed):
    """qkv for ocab_attention.  One key direction per head everywhere, and winners only in the inner (ws/2)^2 of their window, which no
    neighbouring key window reaches: every query window still sees exactly its own winner(s)."""
    inner = [r * ws + c for r in range(ws // 4, ws - ws // 4) for c in range(ws // 4, ws - ws // 4)]
    nw = (H // ws) * (W // ws)
    q, k, v, info = attn_tokens(family, nw, ws * ws, heads, d, seed, logit=OCAB_LOGIT, u_global=True, winners=inner)
    qkv = torch.cat([win_merge(t.reshape(nw, ws * ws, heads * d), ws, ws, H, W) for t in (q, k, v)], dim=-1)
    return qkv.contiguous(), (q, k, v, info)


def naf_tail(g, x, w3, b3, w4, b4, w5, b5, sca, beta, ln_g, ln_b, gamma, dt, eps=1e-6):
    """y = x + beta * conv3(g * sca), then y + gamma * conv5(SimpleGate(conv4(LayerNorm(y))))"""
    y = x.to(dt) + beta.to(dt) * linear(g.to(dt) * sca.to(dt), w3, b3, dt)
    return naf_ffn(y, ln_g, ln_b, w4, b4, w5, b5, gamma, dt, eps)


def band_mha(qkv, P, nb, heads, dt):
    E = qkv.shape[-1] // 3
    d = E // heads
    q, k, v = [t.reshape(P, nb, heads, d).transpose(1, 2) for t in qkv.to(dt).chunk(3, dim=-1)]
    return (torch.softmax((q * d ** -0.5) @ k.transpose(-2, -1), dim=-1) @ v).transpose(1, 2).reshape(P * nb, E)


# ------------------------------------------------------------------------------------------------------------------------------
# statistics of a channel range: the two forms an accumulator-side kernel can take, emulated with fp32 running sums
def stats_f64(v):
    v = v.double()
    mean = v.mean(-1)
    return mean, 1.0 / torch.sqrt(((v - mean[:, None]) ** 2).mean(-1) + 1e-5)


def stats_two_pass_fp32(v, eps=1e-5):
    v = v.float()
    n = v.shape[-1]
    mean = v.sum(-1) / n
    d = v - mean[:, None]
    return mean, 1.0 / torch.sqrt((d * d).sum(-1) / n + eps)


def stats_one_pass_fp32(v, eps=1e-5):
    """var = ssq / n - mean^2 from sequential fp32 running sums, clamped at 0."""
    v = v.float()
    n = v.shape[-1]
    s = torch.zeros(v.shape[0])
    q = torch.zeros(v.shape[0])
    for j in range(n):
        s = s + v[:, j]
        q = q + v[:, j] * v[:, j]
    mean = s / n
    return mean, 1.0 / torch.sqrt((q / n - mean * mean).clamp_min(0.0) + eps)


def _seq_sum(v):
    s = torch.zeros(v.shape[0])
    for j in range(v.shape[-1]):
        s = s + v[:, j]
    return s


def stats_two_pass_seq_fp32(v, eps=1e-5):
    """Two-pass with sequential fp32 running sums over two halves (a lane pair), not ATen's order."""
    v = v.float()
    n, h = v.shape[-1], v.shape[-1] // 2
    mean = (_seq_sum(v[:, :h]) + _seq_sum(v[:, h:])) / n
    d = v - mean[:, None]
    d = d * d
    return mean, 1.0 / torch.sqrt((_seq_sum(d[:, :h]) + _seq_sum(d[:, h:])) / n + eps)


def stats_grouped_fp32(v, eps=1e-5, group=4):
    """token_linear_kernel's form: every value is first shifted by a pivot, the mean of the lane's first group (an exact subtraction
    wherever the row's offset is large against its spread), then groups of four shifted values, each with its own mean and centred sum of squares,
    are merged one after the other with the pairwise update; two lanes take alternate groups and merge at the end, still in the
    shifted domain.  fp32 throughout."""
    v = v.float()
    M, n = v.shape

    def lane(cols):
        cols = list(cols)
        piv = _seq_sum(v[:, cols[0]:cols[0] + group]) * torch.tensor(1.0 / group, dtype=F32)
        cnt, mean, m2 = 0.0, torch.zeros(M), torch.zeros(M)
        for c0 in cols:
            g = v[:, c0:c0 + group] - piv[:, None]
            cn = float(g.shape[-1])
            tm = _seq_sum(g) * torch.tensor(1.0 / cn, dtype=F32)
            d = g - tm[:, None]
            tq = _seq_sum(d * d)
            dl, wn = tm - mean, torch.tensor(cn / (cnt + cn), dtype=F32)
            mean = mean + dl * wn
            m2 = m2 + (tq + dl * dl * torch.tensor(cnt, dtype=F32) * wn)
            cnt += cn
        return cnt, piv, mean, m2
    na, pa, ma, qa = lane(range(0, n, 2 * group))
    nb, pb, mb, qb = lane(range(group, n, 2 * group))
    dl = (pb - pa) + (mb - ma)                       # the lanes merge in the shifted domain: the pivots' difference is exact
    mean = pa + (ma + dl * torch.tensor(nb / n, dtype=F32))
    var = (qa + qb + dl * dl * torch.tensor(na * nb / n, dtype=F32)) / n
    return mean, 1.0 / torch.sqrt(var + eps)


def stats_bars(v, eps=1e-5):
    """-> (mean_ref, rstd_ref, per-row bar on |mean - mean_ref|, bar on the relative rstd error) for values v [M, n]: FACTOR times the
    two-pass fp32 stand-in's error on the same values, the mean with a floor of 2^-22 max(1, |mean|)."""
    mr, rr = stats_f64(v)
    ms, rs = stats_two_pass_fp32(v, eps)
    mean_bar = torch.maximum(torch.full_like(mr, FACTOR * (ms.double() - mr).abs().max().item()), 2.0 ** -22 * mr.abs().clamp_min(1.0))
    rstd_bar = FACTOR * ((rs.double() - rr).abs() / rr).max().item()
    return mr, rr, mean_bar, rstd_bar


# ------------------------------------------------------------------------------------------------------------------------------
# the rule
def family_errors(out, ref64, fam):
    """max |out - ref| / max(1, max|ref|) per family; out / ref64 [M, ...] with the families along dim 0."""
    e = {}
    for name, sl in fam.items():
        r = ref64[sl]
        e[name] = ((out[sl].double() - r).abs().max() / r.abs().max().clamp_min(1.0)).item()
    return e


def check(out, ref64, standin32, fam, bar, name, report=None):
    """Assert the rule on every family; -> {family: (kernel error, allowance)}.  out on any device, ref64 / standin32 on the CPU."""
    out = out.detach().cpu()
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    ke, se = family_errors(out, ref64, fam), family_errors(standin32, ref64, fam)
    res = {f: (ke[f], bar + FACTOR * se[f]) for f in fam}
    if report is not None:
        report[name] = {f: {"err": ke[f], "allow": res[f][1], "standin": se[f]} for f in fam}
    print(f"{name}: " + ", ".join(f"{f} {ke[f]:.2e}/{res[f][1]:.2e}" for f in fam))
    bad = {f: r for f, r in res.items() if not r[0] <= r[1]}
    assert not bad, f"{name}: over the allowance (error, allowance): {bad}"
    return res


ALL = {"all": slice(None)}      # for outputs that are not per row (a pooled vector, a channel matrix)
