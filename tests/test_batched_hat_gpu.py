"""Batched HAT: HatHIP.forward(lr [B,3,h,w]) makes one launch per op for the whole batch and every image comes out with the bits of
its own single forward; FreqFusionHIP.forward / graphed / experts_with_features on top of it.  torch.equal throughout: the contract
is bit identity with the single-image path.  These are also the first tests that run ff_win_attn_fused and ff_ocab_attn with B > 1."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ["bf16x3", "bf16"]


def _lr(seed, B, h, w):
    return torch.from_numpy(np.random.default_rng(seed).random((B, 3, h, w), dtype=np.float32)).cuda()


@pytest.fixture(scope="module")
def model(synth_sd):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd.model import FreqFusionHIP
    return FreqFusionHIP(synth_sd, "cuda:0")


@pytest.fixture(params=MODES)
def mode(request):
    from isr2_amd import ops
    prev = ops.gemm_mode()
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(prev)


def _hat_singles(hat, lr):
    outs, feats = [], []
    for b in range(lr.shape[0]):
        f = {}
        outs.append(hat.forward(lr[b:b + 1].contiguous(), feats=f))
        feats.append(f["hat"])
    return torch.cat(outs), torch.cat(feats)


# B = 3 at 16x16: one window per image, the shifted blocks' mask, the sub-1024-pixel convolution route (implicit GEMM + pool_mean(B) +
# vec_mlp(B)); B = 2 at 32x48: 2x3 windows, the halo route with per-image partials, OCAB with neighbours; B = 2 at 20x40: reflect
# padding to 32x48
@pytest.mark.parametrize("B,h,w", [(3, 16, 16), (2, 32, 48), (2, 20, 40)])
def test_hat_batch_equals_single_forwards(model, mode, B, h, w):
    hat = model.hat
    lr = _lr(100 + h, B, h, w)
    want, want_f = _hat_singles(hat, lr)
    f = {}
    got = hat.forward(lr, feats=f)
    assert tuple(got.shape) == (B, 3, 4 * h, 4 * w) and tuple(f["hat"].shape) == tuple(want_f.shape)
    for b in range(B):
        assert torch.equal(got[b], want[b]), f"image {b}: output"
        assert torch.equal(f["hat"][b], want_f[b]), f"image {b}: conv_after_body feature"
    assert torch.equal(hat.forward(lr), got)                      # the residual form of conv_after_body (no feats)
    assert not torch.equal(got[0], got[1])


def test_hat_launch_count_does_not_scale_with_batch(model, mode, monkeypatch):
    from isr2_amd import ops
    calls = []
    real = ops.win_attn_fused

    def counted(*a, **k):
        calls.append(a[0].shape[0])
        return real(*a, **k)

    monkeypatch.setattr(ops, "win_attn_fused", counted)
    model.hat.forward(_lr(7, 1, 16, 16))
    n1 = len(calls)
    assert n1 == model.hat.groups * model.hat.depth
    del calls[:]
    model.hat.forward(_lr(8, 3, 16, 16))
    assert len(calls) == n1 and set(calls) == {3}


def test_hat_chunked_batch_equals_single_forwards(model, mode, monkeypatch):
    from isr2_amd import ops
    hat = model.hat
    lr = _lr(9, 3, 16, 16)
    want, want_f = _hat_singles(hat, lr)
    calls = []
    real = ops.win_attn_fused

    def counted(*a, **k):
        calls.append(a[0].shape[0])
        return real(*a, **k)

    monkeypatch.setattr(ops, "win_attn_fused", counted)
    monkeypatch.setattr(hat, "max_batch_tokens", 2 * 256)         # the tokens of two images: a chunk of two, then one
    f = {}
    got = hat.forward(lr, feats=f)
    assert sorted(set(calls)) == [1, 2] and len(calls) == 2 * hat.groups * hat.depth
    assert torch.equal(got, want) and torch.equal(f["hat"], want_f)


def test_model_batch_equals_single_forwards_and_graph(model, mode):
    lr = _lr(11, 3, 32, 32)
    want = torch.cat([model(lr[b:b + 1].contiguous()) for b in range(3)])
    got = model(lr)
    assert tuple(got.shape) == (3, 3, 128, 128)
    for b in range(3):
        assert torch.equal(got[b], want[b]), f"image {b}"
    try:
        assert torch.equal(model.graphed(lr), got)
        assert torch.equal(model.graphed(lr), got)                # the replay of the captured graph
    finally:                                                      # the graph cache is keyed by shape, not by contraction mode
        from isr2_amd import ops
        torch.cuda.synchronize()
        for key in list(model._graphs):
            model._graphs.pop(key)
            ops.drop_persistent(key=(id(model),) + key)


@pytest.mark.parametrize("streams", [True, False])
def test_experts_with_features_batch_equals_single_calls(model, mode, streams):
    lr = _lr(12, 2, 16, 16)
    outs, feats = model.experts_with_features(lr, streams=streams)
    assert tuple(outs["hat"].shape) == (2, 3, 64, 64) and tuple(feats["hat"].shape) == (2, 180, 16, 16)
    assert tuple(feats["dat"].shape) == (2, 180, 16, 16) and tuple(feats["nafnet"].shape) == (2, 64, 16, 16)
    for b in range(2):
        o1, f1 = model.experts_with_features(lr[b:b + 1].contiguous(), streams=streams)
        for k in ("hat", "dat", "nafnet"):
            assert torch.equal(outs[k][b:b + 1], o1[k]), f"image {b}: {k} output"
            assert torch.equal(feats[k][b:b + 1], f1[k]), f"image {b}: {k} feature"


def test_plan_recording_refuses_a_batch_of_unaligned_images(model):
    """An image of 3 * 5 * 5 floats does not start on a 16-byte boundary inside its batch; forward() copies it with a torch op, which a
    recorded plan cannot carry, so a recording pass (a marker is installed) must refuse before any launch."""
    from isr2_amd.lib import FFError
    lr = torch.rand(2, 3, 5, 5, device="cuda")
    model._marker = lambda what: None
    try:
        with pytest.raises(FFError):
            model.forward(lr)
    finally:
        model._marker = None
