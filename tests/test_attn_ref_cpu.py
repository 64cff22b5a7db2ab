"""CPU checks of tests/golden/attn_ref.py, the stage-rounded fp64 references tests/test_lowprec_attn_gpu.py holds the plain-bf16 attention
kernels to.  No GPU: an fp32 stand-in of the kernels' ONLINE softmax plays the kernel over the SAME case table the GPU test runs -- fp32
matmul on the bf16-rounded operands, the kernel's tiles walked one after the other with a running maximum and the `o *= corr` rescale,
exp2(fma(s, LOG2E, -m LOG2E)) in fp32 (torch.exp2), a cast to bfloat16 (bf16_rne), the kernel's denominator rule.  The reference is
evaluated in closed form (one pass, exact exp(m_tile - m_final) factors), so the two share the window geometry and nothing of the softmax.

Per kernel and case:
  * the stand-in passes the module's assertion; both caps hold (stage_ref.assert_caps), computed from the reference alone; for the
    fixed-point cases of the fused kernel the exactness assertions hold (attn_ref.assert_exact);
  * every REQUIRED mutant of the stand-in FAILS the assertion on every case it applies to:
        drop      a. one key dropped (its P set to 0)
        swap      b. the bias gathered with q and k exchanged
        off       b. the bias gathered one table entry off for query row 5
        nomask    c. the mask omitted (cases with a mask)
        nopad     d. OCAB: zero keys outside the image removed from the softmax (every OCAB window here touches a border)
        den       e. the denominator rule exchanged (rounded <-> unrounded)
        trunc     f. P truncated instead of rounded to nearest -- required for the kernels with the UNROUNDED denominator (window_attn, the
                     d == 32 fused case); reported only where the denominator sums the same truncated P and the bias largely cancels
        final     g. P rounded relative to the FINAL row maximum instead of the running one -- required on the sharpened cases, reported on
                     the others
        tail0     h. the tail keys of the ragged 576-key chunk scored 0 instead of -inf (window_attn on OCAB keys)
        chan      i. the q head slice shifted by one channel
    c's second form, the mask applied as -inf instead of -100, is NOT in the list: it differs from the reference only where a query has a
    same-region key scoring below about -80, which no case has (e^-100 = 4e-44 of the row maximum is far below the fp32 bound), so it
    is dropped rather than a case contrived for it.

Measured here (ATTN_REF_WORST, printed at teardown; err and err - allow as fractions of max(1, max|ref|), the largest shares over a
kernel's cases; figures rounded):
    ocab_attn       err 3.2e-03 (a bf16 output that rounded the other way), err - allow 4.8e-07, wide 0.0087, fragile P 0.0063
    win_attn_fused  err 4.2e-03 (same), err - allow 3.1e-07, wide 0.0229, fragile P 0.0072
    window_attn     err 5.5e-04, err - allow 9.0e-07, wide 0.0092, fragile P 0.0074
No row is wide throughout; mean allowances are 8e-6 .. 9e-5.  Every required mutant is rejected by at least 7 x the bound: the weakest
are one dropped key in a sharpened OCAB case (7.5 x; the key carries little weight there) and the denominator exchange (9.5 x); the
others by 30 x (final) to 20 000 x (chan).  trunc is also rejected by every rounded-denominator case (at least 32 x the bound) though
not required there.  final is rejected on every flat case too, except window_attn's one-window 16x16 shift-8 cases: each mask region
lies inside one 128-key chunk there, every key that is not masked is rounded at the final maximum already and the mutant differs by
e^-100, so it is reported only for those, sharpened or not; the sharpened 32x48, DAT and OCAB cases carry the requirement."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import attn_ref as A  # noqa: E402
import lowprec_ref as R  # noqa: E402

LOG2E = torch.tensor(1.4426950408889634, dtype=torch.float32)
ALL = [(k, c) for k, cases in A.CASES.items() for c in cases]
WORST = {}


@pytest.fixture(scope="module")
def report():
    yield
    print("\nATTN_REF_WORST " + " ".join(f"{k}: err {v['err']:.2e} err-allow {v['exc']:.2e} wide {v['wide']:.4f} fragile {v['fragile']:.4f};"
                                         for k, v in sorted(WORST.items())))


def fma32(a, b, c):
    """fp32 fma: the product of two floats is exact in fp64; one rounding to fp32 (the fp64 sum's own rounding is 2^-29 below it)."""
    return (a.double() * b.double() + c.double()).float()


def standin(pb: A.Problem, mut=None):
    """The online softmax in fp32 -> [ntok, heads * d] fp32 (bf16 values where the kernel stores bf16)."""
    q, k, v = pb.q.float(), pb.k.float(), pb.v.float()
    G, Q, Nk = pb.bias.shape
    s = q.matmul(k.transpose(1, 2)) + pb.bias.float()
    if pb.smask is not None:
        s = s + pb.smask.float()
    s = s + pb.neg.float()
    live = pb.live.expand(G, Q, Nk)
    s = torch.where(live, s, torch.zeros(()) if mut == "tail0" else torch.full((), -float("inf")))
    alive = live if mut != "tail0" else torch.ones_like(live)
    den_rounded = pb.den_rounded != (mut == "den")
    rnd_ = R.bf16_trunc if mut == "trunc" else R.bf16_rne
    o = torch.zeros(G, Q, pb.d)
    l_run = torch.zeros(G, Q, 1)
    m_run = torch.full((G, Q, 1), -float("inf"))
    m_fin = s.amax(-1, keepdim=True)
    for t0 in range(0, Nk, pb.tile):
        st, lv = s[..., t0:t0 + pb.tile], alive[..., t0:t0 + pb.tile]
        m_new = m_fin if mut == "final" else torch.maximum(m_run, st.amax(-1, keepdim=True))
        have = torch.isfinite(m_new)                                      # (only the nopad mutant can start with a tile without a key)
        m_safe = torch.where(have, m_new, torch.zeros(()))
        corr = torch.where(torch.isfinite(m_run), torch.exp2((m_run - m_safe) * LOG2E), torch.zeros(()))
        e = torch.where(lv, torch.exp2(fma32(torch.where(lv, st, m_safe), LOG2E, -m_safe * LOG2E)), torch.zeros(()))
        p = rnd_(e.contiguous())
        if mut == "drop" and t0 == 0:
            p = p.clone()
            p[..., 3] = 0.0
        o = o * corr + p.matmul(v[:, t0:t0 + pb.tile])
        l_run = l_run * corr + (p if den_rounded else e).sum(-1, keepdim=True)
        m_run = m_new
    out = o * (1.0 / l_run)
    if pb.out_bf16:
        out = R.bf16_rne(out.contiguous())
    nwin = pb.qtok.shape[0]
    rows = out.reshape(nwin, pb.heads, Q, pb.d).permute(0, 2, 1, 3).reshape(nwin * Q, pb.heads * pb.d)
    tok = pb.qtok.reshape(-1)
    res = torch.zeros(pb.ntok, pb.heads * pb.d)
    res[tok[tok >= 0]] = rows[tok >= 0]
    return res.reshape(1, pb.ntok, -1)


def _mutants(kernel, case, inp):
    """[(name, problem kwargs, stand-in mutation, required)]"""
    unrounded = kernel == "window_attn" or (kernel == "win_attn_fused" and case["d"] == 32)
    # the one-window 16x16 shift-8 case of window_attn: each of the four 8x8 regions lies inside ONE 128-key chunk, so every key that is not
    # masked is rounded at the final maximum already -- the mutant differs by e^-100 there, by the arithmetic; reported only
    sharp = bool(case.get("sharp")) and not (kernel == "window_attn" and case["kind"] == "hat" and case["H"] == 16)
    ms = [("drop", {}, "drop", True), ("swap", dict(bias_mut="swap"), None, True), ("off", dict(bias_mut="off"), None, True),
          ("den", {}, "den", True), ("trunc", {}, "trunc", unrounded), ("final", {}, "final", sharp), ("chan", dict(chan_mut=1), None, True)]
    if inp.get("use_mask"):
        ms.append(("nomask", dict(mask_mut="omit"), None, True))
    if kernel == "ocab_attn":
        ms.append(("nopad", dict(pad_mut="remove"), None, True))
    if kernel == "window_attn" and case["kind"] == "ocab":
        ms.append(("tail0", {}, "tail0", True))
    return ms


@pytest.mark.parametrize("kernel,case", ALL, ids=[f"{k}-{A.case_name(c)}".replace(" ", "-") for k, c in ALL])
def test_standin_passes_mutants_fail_and_caps_hold(kernel, case, report):
    inp, sr, info = A.reference(kernel, case)
    name = f"{kernel} [{A.case_name(case)}]"
    shares = A.assert_caps(sr, name)                                      # from the reference alone, before any output is looked at
    if kernel == "win_attn_fused":
        A.assert_exact(info["facts"], name)
    out = standin(A.PROBLEMS[kernel](**inp))
    err, exc = A.compare(out, sr)
    print(f"ATTN_REF_STANDIN {name}: err {err:.3e}, err - allow {exc:.3e} of max(1, max|ref| = {sr.ref.abs().max().item():.3f}); wide "
          f"{shares['wide']:.4f}, fragile P {info['fragile']:.4f}, mean allowance {sr.allow.mean().item():.2e}")
    w = WORST.setdefault(kernel, dict(err=0.0, exc=-1.0, wide=0.0, fragile=0.0))
    w["err"], w["exc"], w["wide"], w["fragile"] = max(w["err"], err), max(w["exc"], exc), max(w["wide"], shares["wide"]), max(w["fragile"], info["fragile"])
    assert exc <= A.FP32_CHAIN_TOL, f"{name}: the fp32 stand-in is outside the bound by {exc:.3e}"
    undetected = []
    for mut, kw, smut, required in _mutants(kernel, case, inp):
        bad = standin(A.PROBLEMS[kernel](**inp, **kw), smut)
        e = A.compare(bad, sr)[1]
        print(f"ATTN_REF_MUTANT {name} {mut}{'' if required else ' (reported only)'}: err - allow {e:.3e} ({e / A.FP32_CHAIN_TOL:.1f} x the bound)")
        if required and e <= A.FP32_CHAIN_TOL:
            undetected.append(mut)
    assert not undetected, f"{name}: mutants the assertion did not reject: {undetected}"


def test_references_match_plain_softmax():
    """Each reference against the UNROUNDED fp64 softmax of the same scores written with torch.softmax: they differ by the rounding of P
    only (2^-9 per probability, averaged over the row) -- a wrong schedule, weight or denominator would be far outside."""
    for kernel, case in ((k, cs[0]) for k, cs in A.CASES.items()):
        inp, sr, _ = A.reference(kernel, case)
        pb = A.PROBLEMS[kernel](**inp)
        s = pb.q.matmul(pb.k.transpose(1, 2)) + pb.bias + pb.neg + (0.0 if pb.smask is None else pb.smask)
        s = torch.where(pb.live.expand_as(s), s, torch.full((), -float("inf"), dtype=torch.float64))
        o = torch.softmax(s, -1).matmul(pb.v)
        nwin, Q = pb.qtok.shape
        rows = o.reshape(nwin, pb.heads, Q, pb.d).permute(0, 2, 1, 3).reshape(nwin * Q, -1)
        tok = pb.qtok.reshape(-1)
        plain = torch.zeros(pb.ntok, pb.heads * pb.d, dtype=torch.float64)
        plain[tok[tok >= 0]] = rows[tok >= 0]
        err = R.rel_err(plain, sr.ref[0])
        print(f"{kernel}: stage-rounded vs unrounded fp64 softmax: {err:.3e} of max(1, max|ref|)")
        assert 1e-7 < err < 4e-3, (kernel, err)


def test_geometry_against_unfold():
    """The window geometry and the bias gather, independently: OCAB's keys against F.unfold (kernel 24, stride 16, padding 4) of a token
    index image, the shifted windows against torch.roll + reshape, and the overlapping-window gather against prep.pack_rel_overlap's
    rotation read the way ocab_attn.hip:80 reads it (i = 600 - 39 qy - qx + 39 ky + kx)."""
    import torch.nn.functional as F
    H, W = 32, 48
    geo = A.geometry(H, W, H, W, 16, 16, 24, 24, 0, 0, False)
    img = torch.arange(1, H * W + 1, dtype=torch.float32).reshape(1, 1, H, W)
    unf = F.unfold(img, kernel_size=24, stride=16, padding=4)[0].t().long() - 1              # [windows, 576], -1 = zero key
    assert torch.equal(unf, geo["ktok"])
    geo = A.geometry(H, W, H, W, 16, 16, 16, 16, 8, 8, True)
    tok = torch.arange(H * W).reshape(H, W).roll((-8, -8), (0, 1))
    win = tok.reshape(H // 16, 16, W // 16, 16).permute(0, 2, 1, 3).reshape(-1, 256)
    assert torch.equal(win, geo["qtok"]) and torch.equal(win, geo["ktok"])
    reg = torch.zeros(H, W, dtype=torch.long)                                                  # the reference models' region image
    for i, ys in enumerate((slice(0, -16), slice(-16, -8), slice(-8, None))):
        for j, xs in enumerate((slice(0, -16), slice(-16, -8), slice(-8, None))):
            reg[ys, xs] = 3 * i + j
    rw = reg.reshape(H // 16, 16, W // 16, 16).permute(0, 2, 1, 3).reshape(-1, 256)
    assert torch.equal(rw[:, :, None] != rw[:, None, :], geo["qreg"][:, :, None] != geo["kreg"][:, None, :])
    sys.path.insert(0, os.path.dirname(HERE))
    from isr2_amd.prep import pack_rel_overlap
    table = A.rnd(39 * 39, 2, seed=5)
    rot = pack_rel_overlap(table, 16, 24)                                                     # [heads, 1521]
    g = A.geometry(16, 16, 16, 16, 16, 16, 24, 24, 0, 0, False)
    mine = A.gather_bias(table.t().contiguous(), 16, 16, 24, 24, g)
    qy, qx, ky, kx = g["qyl"][:, None], g["qxl"][:, None], g["kyl"][None, :], g["kxl"][None, :]
    assert torch.equal(mine, rot[:, 600 - 39 * qy - qx + 39 * ky + kx])
