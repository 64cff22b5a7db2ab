"""Batched NAFNet-SR: NafnetHIP.forward(lr [B,3,h,w]) makes one launch per op for the whole batch and every image comes out with the bits
of its own single forward; FreqFusionHIP.forward / graphed on top of it.  torch.equal throughout: the contract is bit identity with
the single-image path (the per-image loop is reached by slicing the batch)."""
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


def _singles(naf, lr):
    outs, feats = [], []
    for b in range(lr.shape[0]):
        f = {}
        outs.append(naf.forward(lr[b:b + 1].contiguous(), feats=f).clone())
        feats.append(f["nafnet"].clone())
    return torch.cat(outs), torch.cat(feats)


def _check_batch(naf, lr):
    B, _, h, w = lr.shape
    want, want_f = _singles(naf, lr)
    f = {}
    got = naf.forward(lr, feats=f)
    assert tuple(got.shape) == (B, 3, 4 * h, 4 * w) and tuple(f["nafnet"].shape) == tuple(want_f.shape) and want_f.shape[-1] == 64
    for b in range(B):
        assert torch.equal(got[b], want[b]), f"image {b}: output"
        assert torch.equal(f["nafnet"][b], want_f[b]), f"image {b}: feature (the input of the ending convolution)"
    buf = torch.full((B + 1, 3, 4 * h, 4 * w), -1.0, device=lr.device)
    ret = naf.forward(lr, out=buf[1:])                            # out= slices of a larger buffer
    assert ret.data_ptr() == buf[1:].data_ptr() and torch.equal(buf[1:], want) and bool((buf[0] == -1.0).all())
    assert not torch.equal(got[0], got[1]) and not torch.equal(f["nafnet"][0], f["nafnet"][1])


# (3,4,4): HR 16 x 16, the middle level is ONE row per image, so every deep GEMM tile holds all images; sub-1024-pixel conv routes.
# (2,9,13): HR 36 x 52 zero-padded to 48 x 64: the padding region, partial front tiles, the halo route of the ending convolution.
@pytest.mark.parametrize("B,h,w", [(3, 4, 4), (2, 9, 13), (2, 32, 32)])
def test_nafnet_batch_equals_single_forwards(model, mode, B, h, w):
    _check_batch(model.nafnet, _lr(200 + h, B, h, w))


def test_nafnet_f32_mode_keeps_the_loop_and_equals_single_forwards(model):
    from isr2_amd import ops
    prev = ops.gemm_mode()
    ops.set_gemm_mode("f32")
    try:
        _check_batch(model.nafnet, _lr(231, 2, 4, 4))
    finally:
        ops.set_gemm_mode(prev)


def _count_vec_mlp(monkeypatch, calls):
    from isr2_amd import ops
    real = ops.vec_mlp

    def counted(v, *a, **k):
        calls.append(tuple(v.shape) if isinstance(v, torch.Tensor) else (v.images, v.C))     # (HAT hands over PoolPartials)
        return real(v, *a, **k)

    monkeypatch.setattr(ops, "vec_mlp", counted)


def test_nafnet_launch_count_does_not_scale_with_batch(model, mode, monkeypatch):
    naf = model.nafnet
    calls = []
    _count_vec_mlp(monkeypatch, calls)
    naf.forward(_lr(7, 1, 4, 4))
    assert len(calls) == 36 == sum(naf.enc_n) + naf.mid_n + sum(naf.dec_n) and {c[0] for c in calls} == {1}
    del calls[:]
    naf.forward(_lr(8, 3, 4, 4))
    assert len(calls) == 36 and {c[0] for c in calls} == {3}


def test_nafnet_chunked_batch_equals_single_forwards(model, mode, monkeypatch):
    naf = model.nafnet
    lr = _lr(9, 3, 4, 4)
    want, want_f = _singles(naf, lr)
    calls = []
    _count_vec_mlp(monkeypatch, calls)
    monkeypatch.setattr(naf, "max_batch_pixels", 2 * 16 * 16)     # the padded HR pixels of two images: a chunk of two, then one
    f = {}
    got = naf.forward(lr, feats=f)
    assert [c[0] for c in calls] == [2] * 36 + [1] * 36
    assert torch.equal(got, want) and torch.equal(f["nafnet"], want_f)
    assert not torch.equal(got[0], got[2])


def test_model_batch_equals_single_forwards_and_graph(model, mode, monkeypatch):
    calls = []
    _count_vec_mlp(monkeypatch, calls)
    lr = _lr(11, 3, 32, 32)
    want = torch.cat([model(lr[b:b + 1].contiguous()) for b in range(3)])
    del calls[:]
    got = model(lr)
    assert sum(1 for c in calls if c[0] == 3 and c[1] in (64, 128, 256, 512, 1024)) >= 36      # NAFNet ran as one batch inside the model
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
