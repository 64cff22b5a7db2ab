"""LiveEpoch(color_jitter=...) on the GPU: a folder of four seeded PNG pairs just above the 16-pixel patch, B = 2, synthetic weights.
Bit comparisons: color_jitter=None against a LiveEpoch built without the argument; with jitter, micro-batch 0 against sample_pairs_u8 ->
color_jitter_pairs -> experts_with_features done by hand (and against the numpy restatement of the jitter); overlap on against off; the
same epoch asked for twice."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import jitter_ref as J  # noqa: E402

EXPERTS = ("hat", "dat", "nafnet")
LR_SIZES = {"a0": (18, 21), "b1": (17, 16), "c2": (16, 19), "d3": (20, 17)}
PATCH = 16
JIT = dict(prob=0.6, brightness=0.2, contrast=0.2, saturation=0.2)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def pool(tmp_path_factory):
    _need_gpu()
    from PIL import Image
    from isr2_amd import epoch as E
    root = tmp_path_factory.mktemp("livejit")
    rng = np.random.default_rng(78)
    hr_dir, lr_dir = os.path.join(str(root), "hr"), os.path.join(str(root), "lr")
    os.makedirs(hr_dir)
    os.makedirs(lr_dir)
    for stem, (h, w) in LR_SIZES.items():
        lr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        hr = np.repeat(np.repeat(lr, 4, axis=0), 4, axis=1) ^ rng.integers(0, 32, (4 * h, 4 * w, 3), dtype=np.uint8)
        Image.fromarray(lr).save(os.path.join(lr_dir, stem + ".png"))
        Image.fromarray(hr).save(os.path.join(hr_dir, stem + ".png"))
    return E.ImagePool(hr_dir, lr_dir, patch=PATCH, readers=2)


@pytest.fixture(scope="module")
def model(synth_sd):
    _need_gpu()
    from isr2_amd.model import FreqFusionHIP
    return FreqFusionHIP(synth_sd, "cuda:0")


def _collect(data, epoch):
    return [[t.clone() for t in (lr, hr, *(outs[k] for k in EXPERTS), *(feats[k] for k in EXPERTS))] for lr, hr, outs, feats in data.batches(epoch)]


def _same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(torch.equal(s, t) for s, t in zip(x, y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def runs(pool, model):
    """Epoch 0 of every form, once: plain (no argument), color_jitter=None, jitter with one lane, jitter with two (epoch 0 twice)."""
    from isr2_amd import epoch as E
    out = {}
    for name, kw in (("plain", {}), ("none", dict(color_jitter=None)), ("jit1", dict(color_jitter=JIT, overlap=False)),
                     ("jit2", dict(color_jitter=JIT, overlap=True))):
        data = E.LiveEpoch(model, pool, batch_size=2, repeat_factor=2, augment=True, seed=13, **kw)
        try:
            out[name] = _collect(data, 0)
            if name == "jit2":
                out["jit2_again"] = _collect(data, 0)
                out["jit2_epoch1"] = _collect(data, 1)
                out["desc"], out["table"] = data.descriptors(0), data.jitter_table(0)
            if name == "none":
                assert data.jitter_table(0) is None
        finally:
            data.close()
    return out


def test_no_jitter_argument_and_none_give_the_same_bits(runs):
    assert len(runs["plain"]) == 4 and _same(runs["plain"], runs["none"])


def test_micro_batch_zero_is_sampler_jitter_experts_by_hand(runs, pool, model):
    from isr2_amd import epoch as E
    from isr2_amd import ops
    desc, table = runs["desc"], runs["table"]
    assert table.shape == (4, 2, 4) and np.array_equal(table, E.live_jitter_plan(4, 2, 13, 0, **JIT))
    assert 0 < table[..., 0].sum() < 8                                  # the epoch has jittered and untouched samples
    for b in range(4):
        lr, hr = ops.sample_pairs_u8(pool.buf, desc[b], PATCH)
        assert torch.equal(lr, runs["plain"][b][0]) and torch.equal(hr, runs["plain"][b][1])       # the same crops as without jitter
        want = J.jitter_pairs(lr.cpu().numpy(), hr.cpu().numpy(), table[b])
        ops.color_jitter_pairs(lr, hr, table[b])
        assert torch.equal(lr.cpu(), torch.from_numpy(want[0])) and torch.equal(hr.cpu(), torch.from_numpy(want[1])), b
        got = runs["jit2"][b]
        assert torch.equal(got[0], lr) and torch.equal(got[1], hr), b
        for j in range(2):
            if table[b, j, 0] == 0:
                assert torch.equal(got[0][j], runs["plain"][b][0][j]) and torch.equal(got[2][j], runs["plain"][b][2][j])
            else:
                assert not torch.equal(got[0][j], runs["plain"][b][0][j])
        if b == 0:
            outs, feats = model.experts_with_features(lr.clone())
            for k, name in enumerate(EXPERTS):
                assert torch.equal(got[2 + k], outs[name]) and torch.equal(got[5 + k], feats[name]), name


def test_overlap_on_and_off_give_equal_bits(runs):
    assert _same(runs["jit1"], runs["jit2"])


def test_the_same_epoch_twice_gives_equal_bits_and_another_epoch_differs(runs):
    assert _same(runs["jit2"], runs["jit2_again"])
    assert not _same(runs["jit2"], runs["jit2_epoch1"])


def test_color_jitter_argument_is_checked(pool, model):
    from isr2_amd import epoch as E
    from isr2_amd.lib import FFError
    for bad in (dict(hue=0.1), dict(prob=2.0), dict(saturation=1.0)):
        with pytest.raises(FFError):
            E.LiveEpoch(model, pool, batch_size=2, color_jitter=bad)
