"""cache.build_from_folders(batch=N): the patches of an image go through the expert pass in groups of N (HAT batched, a graph per group
size) and every file holds the bits batch=1 writes."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAIRS = (("a_wide", 23, 37), ("b_one", 16, 16))


def _u8(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def model(synth_sd):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import ops
    from isr2_amd.model import FreqFusionHIP
    ops.set_gemm_mode("bf16x3")
    return FreqFusionHIP(synth_sd, "cuda:0")


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("pairs")
    os.makedirs(root / "lr")
    os.makedirs(root / "hr")
    for i, (stem, h, w) in enumerate(PAIRS):
        Image.fromarray(_u8(10 + i, h, w)).save(str(root / "lr" / f"{stem}.png"))
        Image.fromarray(_u8(20 + i, 4 * h, 4 * w)).save(str(root / "hr" / f"{stem}.png"))
    return root


@pytest.fixture(scope="module")
def reference(model, folders, tmp_path_factory):
    """batch=1, built once and shared by both cases."""
    from isr2_amd import cache
    out = str(tmp_path_factory.mktemp("ref"))
    res = cache.build_from_folders(model, str(folders / "hr"), out, lr_dir=str(folders / "lr"), patch=16, crops=3, seed=3, batch=1)
    assert res["batch"] == 1 and res["patches_written"] == 6
    return out


def _assert_same(a, b, where):
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), where
        for k in a:
            _assert_same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    else:
        assert a == b, where


@pytest.mark.parametrize("graph", [True, False])
def test_batched_build_writes_the_files_of_batch_1(model, folders, reference, tmp_path, monkeypatch, graph):
    from isr2_amd import cache
    sizes = []
    real = model.experts_with_features

    def counted(lr, **k):
        sizes.append(lr.shape[0])
        return real(lr, **k)

    monkeypatch.setattr(model, "experts_with_features", counted)
    out = str(tmp_path / "built")
    res = cache.build_from_folders(model, str(folders / "hr"), out, lr_dir=str(folders / "lr"), patch=16, crops=3, seed=3, batch=2, graph=graph)
    assert res["batch"] == 2 and res["graph"] is graph and res["images"] == 2 and res["patches_written"] == 6
    # three patches per image: one full group of two and a remainder of one (graph: a warm-up and a capture per group size)
    assert sizes == ([1, 1, 2, 2] if graph else [2, 1, 2, 1]), sizes
    stems = [f"{s}_p{k}" for s, _, _ in PAIRS for k in range(3)]
    assert cache.list_stems(out) == sorted(stems) == cache.list_stems(reference)
    for s in stems:
        for suf in (cache.PRIMARY_SUFFIX, cache.REST_SUFFIX):
            got = torch.load(os.path.join(out, s + suf), weights_only=True)
            want = torch.load(os.path.join(reference, s + suf), weights_only=True)
            _assert_same(got, want, s + suf)


def test_batch_must_be_positive(model, folders, tmp_path):
    from isr2_amd import cache
    from isr2_amd.lib import FFError
    with pytest.raises(FFError):
        cache.build_from_folders(model, str(folders / "hr"), str(tmp_path / "o"), lr_dir=str(folders / "lr"), patch=16, crops=3, batch=0)
