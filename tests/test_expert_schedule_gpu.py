"""The expert schedule of FreqFusionHIP and the trunk HAT and DAT share: what a host refactor must keep.  Where the plan markers are
emitted, B == 1 as a batch of one, the experts() contract, the hooked-feature form of both trunks, and the lazily packed weights
(made once, under the keys a recorded plan names its slots by).  torch.equal throughout; 16x16 is one HAT window (DAT's 8x32 / 32x8
windows pad it to 32), 20x40 takes every padding rule, B == 2 the per-image loop and the out[b:b+1] slices."""
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


def test_markers_surround_the_three_stream_forward_only(model):
    """A plan recording is told about the fork / join of forward()'s three-stream section, once per forward whatever B is; the
    one-stream schedule, the taps route and experts_with_features emit nothing."""
    one, two = _lr(1, 1, 16, 16), _lr(2, 2, 16, 16)
    seen = []

    def marks(fn):
        del seen[:]
        fn()
        return list(seen)

    ms = model.multi_stream
    model._marker = seen.append
    try:
        model.multi_stream = True
        assert marks(lambda: model.forward(one)) == ["fork", "join"]
        assert marks(lambda: model.forward(two)) == ["fork", "join"]
        assert marks(lambda: model.forward(one, taps={})) == []
        assert marks(lambda: model.experts_with_features(one, streams=True)) == []
        model.multi_stream = False
        assert marks(lambda: model.forward(one)) == []
        assert marks(lambda: model.forward(two)) == []
        assert marks(lambda: model.forward(one, taps={})) == []
    finally:
        model._marker = None
        model.multi_stream = ms
    torch.cuda.synchronize()


def test_single_image_is_a_batch_of_one(model, mode):
    lr = _lr(3, 1, 20, 40)                                        # reflect padding for HAT and DAT, zero padding for NAFNet
    want = model(lr)
    assert tuple(want.shape) == (1, 3, 80, 160)
    out = torch.empty_like(want)
    got = model(lr, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, want)
    both = model(torch.cat([lr, lr]))
    assert tuple(both.shape) == (2, 3, 80, 160)
    assert torch.equal(both[0:1], want) and torch.equal(both[1:2], want)


@pytest.mark.parametrize("multi", [True, False])
def test_experts_contract(model, mode, multi):
    lr = _lr(4, 1, 16, 16)
    ms = model.multi_stream
    model.multi_stream = multi
    try:
        with torch.no_grad():
            ex = model.experts(lr)
            assert sorted(ex) == ["dat", "hat", "nafnet"] and all(tuple(v.shape) == (1, 3, 64, 64) for v in ex.values())
            ex2, pre = model.experts(lr, with_pre=True)
            assert isinstance(pre, dict) if multi else pre is None
            for k in ex:
                assert torch.equal(ex2[k], ex[k]), k
            got = model.fusion.forward(lr, ex2, pre=pre)
        assert torch.equal(got, model(lr))
    finally:
        model.multi_stream = ms


@pytest.mark.parametrize("name", ["hat", "dat"])
def test_trunk_hooked_feature_form_equals_residual_form(model, mode, name):
    """conv_after_body with the residual in its epilogue, or as the hooked feature plus a separate add: the same SR output."""
    net = getattr(model, name)
    lr = _lr(5, 1, 16, 16)
    f = {}
    assert torch.equal(net.forward(lr), net.forward(lr, feats=f))
    assert list(f) == [name] and tuple(f[name].shape) == (1, 16, 16, 180)


def test_lazy_packs_are_made_once_under_their_plan_names(model):
    from isr2_amd import ops
    prev = ops.gemm_mode()
    ops.set_gemm_mode("bf16x3")
    try:
        lr = _lr(6, 1, 16, 16)
        naf = model.nafnet
        dicts = ([blk for g in model.hat.blocks for blk in g] + list(model.hat.ocab) + [blk for g in model.dat.blocks for blk in g]
                 + [k for lvl in naf.encs + naf.decs for k in lvl] + list(naf.mids))

        def keys():
            return [tuple(d) for d in dicts]

        model(lr)
        first = keys()
        model(lr)
        assert keys() == first
        # the spellings are the weight slot names of a recorded plan (plan._walk_tensors)
        assert {"relp", "qkv_wf", "projmlp_pk"} <= set(model.hat.blocks[0][0])
        assert {"qkv_tl", "projmlp_pk"} <= set(model.hat.ocab[0])
        assert {"relp", "qkv_wf", "gp_pk", "fc1_tl"} <= set(model.dat.blocks[0][0])        # a spatial block
        assert {"cq_pk", "gp_pk", "fc1_tl"} <= set(model.dat.blocks[0][1])                 # a channel block
        assert {"c1_tl", "ffn_pk"} <= set(naf.encs[0][0]) and "c4i" in naf.mids[0]
    finally:
        ops.set_gemm_mode(prev)
