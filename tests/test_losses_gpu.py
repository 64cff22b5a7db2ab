"""The loss components of csrc/sr_losses.hip (isr2_amd.autograd.SRLoss) against the reference's own loss classes
(tests/golden/losses.npz, made by tests/golden/make_golden_losses.py from perceptual_loss.py).

Bars, set from the arithmetic:
- value, 1e-5 relative: every value is a fp32 mean of <= 3.1 M terms.  The kernels add in a fixed tree (per-thread grid-stride runs,
  a 256-way tree, a tree over <= 12288 partials), whose error is ~log2(n) ulp ~ 1.3e-6 relative; the reference's own sum (ATen's
  pairwise / cuDNN-free CPU convolution) carries about as much.  The transforms before the sums (11x11 separable Gaussian vs the
  reference's 121-tap 2-D window, a direct DFT vs pocketfft) add a few ulp per term, which the mean averages down.
- gradient, 1e-4 of max|ref| per component: l1 / charbonnier / l2 / edge / swt gradients are signs or single products times fixed
  weights -- exact up to an ulp unless a difference rounds across zero (probability ~1e-7 per term); SSIM's coefficient maps
  differ from autograd's chain by reassociation (~10 ulp of the largest term).  FFT: the phase term's gradient at a bin is
  0.1 w / (N |z|) -- it grows as 1/|z| where the spectrum is small -- and the DFT's absolute error there (~1e-7 |x| sqrt(H + W)) is a
  relative error ~1e-7 sqrt(H+W) / |z| of that bin's share; over the seeded draws the smallest |z| is ~1e-3 of the typical bin,
  which keeps it at ~1e-5 of max|ref| for the two small draws.  The B=16 draw has 250x more bins, so its smallest |z| is ~16x
  smaller (the minimum of n Rayleigh draws scales as 1/sqrt(n)): the 1/|z| phase gradient of that bin carries a relative error
  ~2e-3 (1e-6 rms DFT error over |z| ~ 5.7e-4 rms), and its share of max|ref| sets the deviation -- bounded by 1e-3, which is the
  FFT bar of that case alone (FFT_B16_GRAD_BAR).  Every other component / case keeps 1e-4."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
COMPONENTS = ("l1", "charbonnier", "l2", "ssim", "edge", "fft", "swt")
STAGES = {1: {"l1": 1.0}, 2: {"l1": 0.75, "swt": 0.20, "fft": 0.05}, 3: {"l1": 0.60, "swt": 0.25, "fft": 0.10, "ssim": 0.05}}
CASES = ("b2_64", "b1_72x40", "b16_256")
VALUE_BAR, GRAD_BAR = 1e-5, 1e-4
FFT_B16_GRAD_BAR = 1e-3


@pytest.fixture(scope="module")
def gold():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return np.load(os.path.join(GOLD, "losses.npz"))


@pytest.fixture(scope="module")
def srloss():
    from isr2_amd.autograd import SRLoss
    return SRLoss("cuda:0")


def _inputs(g, case):
    """The fixture's own draw (make_golden_losses.loss_inputs), as NHWC device tensors."""
    meta = json.loads(str(g[f"{case}/meta"]))
    B, H, W = meta["B"], meta["H"], meta["W"]
    rng = np.random.default_rng(meta["seed"])
    pred = (rng.random((B, 3, H, W), dtype=np.float32) * np.float32(1.1) - np.float32(0.05)).astype(np.float32)
    target = rng.random((B, 3, H, W), dtype=np.float32)
    assert np.allclose([pred.astype(np.float64).sum(), target.astype(np.float64).sum()], g[f"{case}/input_sums"], rtol=0, atol=1e-6)
    nhwc = lambda a: torch.from_numpy(a).permute(0, 2, 3, 1).contiguous().cuda()
    return nhwc(pred), nhwc(target), meta


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("comp", COMPONENTS)
def test_component_against_reference(gold, srloss, case, comp):
    sr, hr, meta = _inputs(gold, case)
    dsr = torch.full_like(sr, 7.0)                                    # accumulate = 0 must overwrite
    v = float(srloss.component(comp, sr, hr, 1.0, dsr).cpu())
    ref = float(gold[f"{case}/{comp}/value"])
    g = dsr.reshape(-1).cpu().numpy()
    if meta["full"]:
        gref, got = gold[f"{case}/{comp}/grad"], g
    else:
        gref, got = gold[f"{case}/{comp}/val"], g[gold[f"{case}/{comp}/idx"]]
    gmax = float(gold[f"{case}/{comp}/grad_maxabs"])
    dev = float(np.abs(got - gref).max()) / gmax
    l2 = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    print(f"{case} {comp}: value {v:.8f} ref {ref:.8f} rel {abs(v - ref) / abs(ref):.2e}; grad dev {dev:.2e} of max|ref|; "
          f"l2 {l2:.6e} ref {float(gold[f'{case}/{comp}/grad_l2']):.6e}")
    assert abs(v - ref) <= VALUE_BAR * abs(ref)
    bar = FFT_B16_GRAD_BAR if (comp, case) == ("fft", "b16_256") else GRAD_BAR
    assert dev < bar
    assert abs(l2 - float(gold[f"{case}/{comp}/grad_l2"])) <= bar * float(gold[f"{case}/{comp}/grad_l2"]) * 10


def _combined(srloss, weights, sr, hr, dsr):
    from isr2_amd.autograd import LOSS_ORDER
    active = [(k, weights[k]) for k in LOSS_ORDER if weights.get(k, 0) > 0]
    vals = torch.zeros(len(LOSS_ORDER), device="cuda:0")
    w = torch.tensor([x for _, x in active], dtype=torch.float32, device="cuda:0")
    total = torch.zeros(1, device="cuda:0")
    srloss.combined(active, sr, hr, dsr, vals, w, total)
    return total


@pytest.mark.parametrize("case", CASES)
def test_stage_totals(gold, srloss, case):
    sr, hr, _ = _inputs(gold, case)
    for s, w in STAGES.items():
        dsr = torch.empty_like(sr)
        tot = float(_combined(srloss, w, sr, hr, dsr).cpu())
        ref = float(gold[f"{case}/stage{s}"])
        print(case, "stage", s, tot, ref)
        assert abs(tot - ref) <= VALUE_BAR * abs(ref), (s, tot, ref)


def test_stage3_gradient_is_bit_identical_across_calls(gold, srloss):
    sr, hr, _ = _inputs(gold, "b2_64")
    a, b = torch.empty_like(sr), torch.empty_like(sr)
    ta = _combined(srloss, STAGES[3], sr, hr, a).clone()
    tb = _combined(srloss, STAGES[3], sr, hr, b).clone()
    assert torch.equal(a, b) and torch.equal(ta, tb)


def test_weighted_gradients_add_up(gold, srloss):
    """accumulate = 1 adds weight * gradient: the stage-3 gradient is the weighted sum of the per-component gradients."""
    sr, hr, _ = _inputs(gold, "b1_72x40")
    tot = torch.empty_like(sr)
    _combined(srloss, STAGES[3], sr, hr, tot)
    ref = torch.zeros_like(sr)
    for k, w in STAGES[3].items():
        gk = torch.empty_like(sr)
        srloss.component(k, sr, hr, 1.0, gk)
        ref += w * gk
    assert float((tot - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_zero_weight_component_launches_nothing(gold, srloss, monkeypatch):
    from isr2_amd import lib as L
    sr, hr, _ = _inputs(gold, "b1_72x40")
    real = L.load()
    calls = []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(L, "_lib", Spy())
    a, b = torch.empty_like(sr), torch.empty_like(sr)
    ta = _combined(srloss, {"l1": 0.6, "fft": 0.1, "ssim": 0.0, "edge": 0.0}, sr, hr, a).clone()
    launched = [c for c in calls if c.startswith("ff_loss_")]
    calls.clear()
    tb = _combined(srloss, {"l1": 0.6, "fft": 0.1}, sr, hr, b).clone()
    assert "ff_loss_ssim" not in launched and "ff_loss_edge" not in launched
    assert launched == [c for c in calls if c.startswith("ff_loss_")]
    assert torch.equal(a, b) and torch.equal(ta, tb)
