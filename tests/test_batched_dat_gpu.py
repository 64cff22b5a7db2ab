"""Batched DAT: DatHIP.forward(lr [B,3,h,w]) makes one launch per op for the whole batch and every image comes out with the bits of its
own single forward; FreqFusionHIP.forward / graphed and experts_with_features on top of it.  torch.equal throughout: the contract is bit
identity with the single-image path (the per-image loop is reached by slicing the batch)."""
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


def _singles(dat, lr):
    outs, feats = [], []
    for b in range(lr.shape[0]):
        f = {}
        outs.append(dat.forward(lr[b:b + 1].contiguous(), feats=f).clone())
        feats.append(f["dat"].clone())
    return torch.cat(outs), torch.cat(feats)


def _check_batch(dat, lr):
    B, _, h, w = lr.shape
    want, want_f = _singles(dat, lr)
    f = {}
    got = dat.forward(lr, feats=f)
    assert tuple(got.shape) == (B, 3, 4 * h, 4 * w) and tuple(f["dat"].shape) == tuple(want_f.shape) and want_f.shape[-1] == 180
    for b in range(B):
        assert torch.equal(got[b], want[b]), f"image {b}: output"
        assert torch.equal(f["dat"][b], want_f[b]), f"image {b}: feature (conv_after_body's output)"
    buf = torch.full((B + 1, 3, 4 * h, 4 * w), -1.0, device=lr.device)
    ret = dat.forward(lr, out=buf[1:])                            # out= slices of a larger buffer
    assert ret.data_ptr() == buf[1:].data_ptr() and torch.equal(buf[1:], want) and bool((buf[0] == -1.0).all())
    assert not torch.equal(got[0], got[1]) and not torch.equal(f["dat"][0], f["dat"][1])


# (3,16,16): windows padded in both directions (8 x 32 and 32 x 8 on 16 x 16), one 256-row block per image.
# (2,20,40): reflect padding to 32 x 48, zero-padded windows (Wp 48 -> 64).
# (2,32,32): 1 024 pixels per image, the LDS-resident 3x3 route.
@pytest.mark.parametrize("B,h,w", [(3, 16, 16), (2, 20, 40), (2, 32, 32)])
def test_dat_batch_equals_single_forwards(model, mode, B, h, w):
    _check_batch(model.dat, _lr(300 + h, B, h, w))


def test_dat_f32_mode_keeps_the_loop_and_equals_single_forwards(model, monkeypatch):
    from isr2_amd import ops
    prev = ops.gemm_mode()
    ops.set_gemm_mode("f32")
    try:
        shapes = []
        real = ops.chan_attn_weights
        monkeypatch.setattr(ops, "chan_attn_weights", lambda qkv, *a, **k: (shapes.append(qkv.shape[0]), real(qkv, *a, **k))[1])
        _check_batch(model.dat, _lr(331, 2, 16, 16))
        assert shapes and set(shapes) == {1}                      # the single-image channel attention, image by image
    finally:
        ops.set_gemm_mode(prev)


def _count_gated(monkeypatch, calls):
    from isr2_amd import ops
    real = ops.token_linear_gated

    def counted(x, x2, pk, cm, *a, **k):
        calls.append(tuple(cm.shape))
        return real(x, x2, pk, cm, *a, **k)

    monkeypatch.setattr(ops, "token_linear_gated", counted)


def test_dat_launch_count_does_not_scale_with_batch(model, mode, monkeypatch):
    dat = model.dat
    calls = []
    _count_gated(monkeypatch, calls)
    dat.forward(_lr(7, 1, 16, 16))
    assert len(calls) == 36 == dat.groups * dat.depth and set(calls) <= {(180,), (1, 180)}
    del calls[:]
    dat.forward(_lr(8, 3, 16, 16))
    assert len(calls) == 36 and set(calls) == {(3, 180)}


def test_dat_chunked_batch_equals_single_forwards(model, mode, monkeypatch):
    dat = model.dat
    lr = _lr(9, 3, 16, 16)
    want, want_f = _singles(dat, lr)
    calls = []
    _count_gated(monkeypatch, calls)
    monkeypatch.setattr(dat, "max_batch_tokens", 2 * 16 * 16)     # the padded tokens of two images: a chunk of two, then one
    f = {}
    got = dat.forward(lr, feats=f)
    assert [c[0] if len(c) == 2 else 1 for c in calls] == [2] * 36 + [1] * 36
    assert torch.equal(got, want) and torch.equal(f["dat"], want_f)
    assert not torch.equal(got[0], got[2])


def test_dat_batch_refuses_taps(model, mode):
    from isr2_amd.lib import FFError
    with pytest.raises(FFError):
        model.dat.forward(_lr(10, 2, 16, 16), taps={})


def test_model_batch_equals_single_forwards_and_graph(model, mode, monkeypatch):
    calls = []
    _count_gated(monkeypatch, calls)
    lr = _lr(11, 3, 32, 32)
    want = torch.cat([model(lr[b:b + 1].contiguous()) for b in range(3)])
    del calls[:]
    got = model(lr)
    assert calls == [(3, 180)] * 36                               # DAT ran as one batch inside the model
    assert tuple(got.shape) == (3, 3, 128, 128)
    for b in range(3):
        assert torch.equal(got[b], want[b]), f"image {b}"
    assert not torch.equal(got[0], got[1])
    try:
        assert torch.equal(model.graphed(lr), got)
        assert torch.equal(model.graphed(lr), got)                # the replay of the captured graph
    finally:                                                      # the graph cache is keyed by shape, not by contraction mode
        from isr2_amd import ops
        torch.cuda.synchronize()
        for key in list(model._graphs):
            model._graphs.pop(key)
            ops.drop_persistent(key=(id(model),) + key)


@pytest.mark.parametrize("streams", [False, True])
def test_experts_with_features_batch_equals_per_image(model, mode, streams, monkeypatch):
    lr = _lr(12, 2, 16, 16)
    singles = [model.experts_with_features(lr[b:b + 1].contiguous(), streams=streams) for b in range(2)]
    torch.cuda.synchronize()
    calls = []
    _count_gated(monkeypatch, calls)
    outs, feats = model.experts_with_features(lr, streams=streams)
    torch.cuda.synchronize()
    assert calls == [(2, 180)] * 36
    for k in ("hat", "dat", "nafnet"):
        for b in range(2):
            assert torch.equal(outs[k][b:b + 1], singles[b][0][k]), f"{k} output, image {b}"
            assert torch.equal(feats[k][b:b + 1], singles[b][1][k]), f"{k} feature, image {b}"
    assert not torch.equal(outs["dat"][0], outs["dat"][1]) and not torch.equal(feats["dat"][0], feats["dat"][1])
