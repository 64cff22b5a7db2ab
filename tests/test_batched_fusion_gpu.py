"""Batched fusion stack: FusionHIP.forward(lr [B,3,h,w], experts [B,3,4h,4w]) makes one launch per op for the whole batch and every
image comes out with the bits of its own single forward; FreqFusionHIP.forward / graphed / plans, the cached-mode forward and
epoch.validate on top of it.  torch.equal throughout: the contract is bit identity with the single-image path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ["bf16x3", "bf16"]


def _rand(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).random(shape, dtype=np.float32)).cuda()


def _experts(seed, B, h, w):
    return {k: _rand(seed + i, B, 3, 4 * h, 4 * w) for i, k in enumerate(("hat", "dat", "nafnet"))}


@pytest.fixture(scope="module")
def fus():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd.fusion import FusionHIP
    from isr2_amd.weights import synth_state_dict
    return FusionHIP(synth_state_dict(1234, parts=("fusion", "collab")), torch.device("cuda:0"))


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


def _sl(d, b):
    return None if d is None else {k: v[b:b + 1] for k, v in d.items()}


def _singles(fus, lr, ex, feats=None):
    return torch.cat([fus.forward(lr[b:b + 1], _sl(ex, b), feats=_sl(feats, b)).clone() for b in range(lr.shape[0])])


def _check_batch(fus, lr, ex, feats=None):
    B, _, h, w = lr.shape
    want = _singles(fus, lr, ex, feats)
    got = fus.forward(lr, ex, feats=feats)
    assert tuple(got.shape) == (B, 3, 4 * h, 4 * w)
    for b in range(B):
        assert torch.equal(got[b], want[b]), f"image {b}"
    assert not torch.equal(got[0], got[1])
    buf = torch.full((B + 2, 3, 4 * h, 4 * w), -1.0, device=lr.device)
    ret = fus.forward(lr, ex, feats=feats, out=buf[1:B + 1])       # out= a slice of a larger buffer
    assert ret.data_ptr() == buf[1:].data_ptr() and torch.equal(buf[1:B + 1], want)
    assert bool((buf[0] == -1.0).all()) and bool((buf[B + 1] == -1.0).all())
    return want


# (3,16,16) HR 64 x 64: the small-channel route; (2,17,19) odd sizes; (2,20,40) non-square; (5,16,16) the HR rows of the batch cross the
# 256 * 64 tile threshold that one image stays below; (2,32,32) the halo route at the LR level
@pytest.mark.parametrize("B,h,w", [(3, 16, 16), (2, 17, 19), (2, 20, 40), (5, 16, 16), (2, 32, 32)])
def test_fusion_batch_equals_single_forwards(fus, mode, B, h, w):
    _check_batch(fus, _rand(300 + B + h, B, 3, h, w), _experts(310 + B + h, B, h, w))


def test_cached_mode_batch_equals_single_forwards(fus, mode):
    B, h, w = 3, 16, 16
    feats = {"hat": _rand(320, B, 180, h, w) - 0.5, "dat": _rand(321, B, 180, h, w) - 0.5, "nafnet": _rand(322, B, 64, h, w) - 0.5}
    lr, ex = _rand(323, B, 3, h, w), _experts(324, B, h, w)
    want = _check_batch(fus, lr, ex, feats)
    assert not torch.equal(want, _singles(fus, lr, ex))          # the collaborative gains are live


class _Counting:
    """The kernel library with every launch (an int entry point whose last parameter is the stream) noted as (name, args)."""

    def __init__(self, real):
        from isr2_amd.lib import parse_header
        self.real, self.calls = real, []
        self.launches = {n for n, (ret, args) in parse_header().items() if ret == "int" and args and args[-1] == "void*"}

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in self.launches:
            return fn

        def counted(*a):
            self.calls.append((name, a))
            return fn(*a)
        return counted


def test_launch_count_does_not_scale_with_batch(fus, mode, monkeypatch):
    from isr2_amd import ops
    h = w = 16
    one, three = (_rand(330, 1, 3, h, w), _experts(331, 1, h, w)), (_rand(334, 3, 3, h, w), _experts(335, 3, h, w))
    fus.forward(*one), fus.forward(*three)                         # lazy weight preparations are launches too: make them first
    cnt = _Counting(ops._L())
    monkeypatch.setattr(ops, "_L", lambda: cnt)
    fus.forward(*one)
    n1, names1 = len(cnt.calls), {n for n, _ in cnt.calls}
    del cnt.calls[:]
    fus.forward(*three)
    n3, names3 = len(cnt.calls), {n for n, _ in cnt.calls}
    assert n1 == n3 and n1 > 100
    per_image = {"ff_dct8_bands", "ff_fft_bands", "ff_fuse_blend"}
    assert per_image <= names1 and not per_image & names3
    assert {n + "_images" for n in per_image} <= names3 and not {n + "_images" for n in per_image} & names1
    blend = [a for n, a in cnt.calls if n == "ff_fuse_blend_images"]
    assert len(blend) == 1 and tuple(blend[0][6:11]) == (3, 4 * h, 4 * w, h, w)
    assert [a[1] for n, a in cnt.calls if n == "ff_fft_bands_images"] == [3]
    assert {a[9] for n, a in cnt.calls if n == "ff_conv2d_bf16s"} >= {3}           # B of the implicit GEMM's 3x3 convolutions


def test_chunked_batch_equals_single_forwards(fus, mode, monkeypatch):
    from isr2_amd import ops
    B, h, w = 3, 16, 16
    lr, ex = _rand(340, B, 3, h, w), _experts(341, B, h, w)
    want = _singles(fus, lr, ex)
    made = []
    real = ops.persistent_zeros

    def noted(owner, role, shape, device):
        buf = real(owner, role, shape, device)
        made.append((role, tuple(shape), buf.data_ptr()))
        return buf

    monkeypatch.setattr(ops, "persistent_zeros", noted)
    monkeypatch.setattr(fus, "max_batch_pixels", 2 * 16 * h * w)    # the HR pixels of two images: a chunk of two, then one
    assert fus._chunk_images(B, h, w) == 2
    blends = []
    real_blend = ops.fuse_blend
    monkeypatch.setattr(ops, "fuse_blend", lambda e9, *a: (blends.append(e9.shape[0]), real_blend(e9, *a))[1])
    got = fus.forward(lr, ex)
    again = fus.forward(lr, ex)
    assert blends == [2, 1, 2, 1]
    assert torch.equal(got, want) and torch.equal(again, want) and not torch.equal(got[0], got[2])
    # the concat buffers are made once, for the largest chunk; the remainder chunk takes a leading slice of the same buffer
    for role, hw in (("in2", (2 * h, 2 * w)), ("in3", (4 * h, 4 * w))):
        seen = [(s, p) for r, s, p in made if r == role]
        assert len(seen) == 4 and len(set(seen)) == 1 and seen[0][0] == (2, *hw, 76), (role, seen)
    # the pre pass run beside the experts is chunked the same way
    pre = fus.pre(lr)
    assert [c["raw"].shape[0] for c in pre["chunks"]] == [2, 1]
    assert torch.equal(fus.forward(lr, ex, pre=pre), want)


def test_f32_mode_keeps_the_loop_and_equals_single_forwards(fus, monkeypatch):
    from isr2_amd import ops
    prev = ops.gemm_mode()
    ops.set_gemm_mode("f32")
    try:
        B, h, w = 2, 16, 16
        lr, ex = _rand(350, B, 3, h, w), _experts(351, B, h, w)
        want = _singles(fus, lr, ex)
        blends = []
        real_blend = ops.fuse_blend
        monkeypatch.setattr(ops, "fuse_blend", lambda e9, *a: (blends.append(e9.shape[0]), real_blend(e9, *a))[1])
        got = fus.forward(lr, ex)
        assert blends == [1, 1] and torch.equal(got, want) and not torch.equal(got[0], got[1])
    finally:
        ops.set_gemm_mode(prev)


def _drop_graphs(model):
    from isr2_amd import ops
    torch.cuda.synchronize()
    for key in list(model._graphs):                               # the graph cache is keyed by shape, not by contraction mode
        model._graphs.pop(key)
        ops.drop_persistent(key=(id(model),) + key)


def test_model_batch_of_odd_images_equals_single_forwards_graph_and_plan(model, mode, tmp_path):
    from isr2_amd import plan
    lr = _rand(360, 3, 3, 17, 19)                                 # 3 * 17 * 19 floats per image: images 1 and 2 are not 16-byte aligned
    assert hasattr(model.fusion, "max_batch_pixels")
    import isr2_amd.model as M
    assert not hasattr(M, "_per_image")
    ms = model.multi_stream
    try:
        model.multi_stream = True
        want = torch.cat([model(lr[b:b + 1].contiguous()) for b in range(3)])
        for multi in (True, False):
            model.multi_stream = multi
            got = model(lr)
            assert tuple(got.shape) == (3, 3, 68, 76)
            for b in range(3):
                assert torch.equal(got[b], want[b]), f"image {b}, multi_stream={multi}"
        assert not torch.equal(want[0], want[1])
        model.multi_stream = True
        try:
            assert torch.equal(model.graphed(lr), want)
            assert torch.equal(model.graphed(lr), want)           # the replay of the captured graph
        finally:
            _drop_graphs(model)
        # a plan recording of that batch: no image is copied outside the tape any more
        seen = []
        model._marker = seen.append
        try:
            assert torch.equal(model.forward(lr), want)
        finally:
            model._marker = None
        assert seen == ["fork", "join"]
        info = plan.export_plan(model, lr, str(tmp_path / "b3_17x19"), verify=True)
        assert info
    finally:
        model.multi_stream = ms
        model._marker = None


def test_forward_with_precomputed_takes_a_batch(mode):
    from isr2_amd.model import FreqFusionHIP
    from isr2_amd.weights import synth_state_dict
    model = FreqFusionHIP(synth_state_dict(1234, parts=("hat", "dat", "nafnet", "fusion", "collab")), "cuda:0")
    B, h, w = 2, 16, 16
    lr = _rand(370, B, 3, h, w)
    outs, feats = model.experts_with_features(lr)
    got = model.forward_with_precomputed(lr, outs, feats)
    assert tuple(got.shape) == (B, 3, 4 * h, 4 * w)
    for b in range(B):
        assert torch.equal(got[b:b + 1], model.forward_with_precomputed(lr[b:b + 1], _sl(outs, b), _sl(feats, b))), f"image {b}"
    plain = model.forward_with_precomputed(lr, outs)
    assert torch.equal(plain, model(lr)) and not torch.equal(plain, got)
    with pytest.raises(Exception):
        model.forward_with_precomputed(lr, _sl(outs, 0), feats)   # expert outputs of another batch size


def test_validate_batch_equals_one_sample_per_forward():
    from isr2_amd import epoch, train
    from isr2_amd.weights import synth_state_dict
    tr = train.FusionTrainer(synth_state_dict(1234, parts=("fusion", "collab")), "cuda:0", gemm="bf16x3")
    h = w = 16
    samples = []
    for i in range(3):
        samples.append(dict(lr=_rand(380 + i, 3, h, w).cpu(), hr=_rand(383 + i, 3, 4 * h, 4 * w).cpu(),
                            expert_imgs={k: v[0].cpu() for k, v in _experts(386 + 3 * i, 1, h, w).items()},
                            expert_feats={"hat": _rand(400 + i, 180, h, w).cpu() - 0.5, "dat": _rand(403 + i, 180, h, w).cpu() - 0.5,
                                          "nafnet": _rand(406 + i, 64, h, w).cpu() - 0.5}))
    one = epoch.validate(tr, samples, return_sr=True)
    two = epoch.validate(tr, samples, return_sr=True, batch=2)    # a group of two, then the remainder
    assert one["per_image"] == two["per_image"] and one["psnr"] == two["psnr"] and one["ssim"] == two["ssim"]
    assert len(two["sr"]) == 3 and all(torch.equal(a, b) for a, b in zip(one["sr"], two["sr"]))
    assert not torch.equal(two["sr"][0], two["sr"][1])
