"""x8 geometric self-ensemble (FreqFusionHIP.self_ensemble, the plugin's FF_SELF_ENSEMBLE switch) on the GPU.  The definition is
pinned bit for bit against torch's own flip / rot90 / add applied to the same forwards, in the stated order:

    acc = inv_0(run(T_0(lr)));  acc = acc + inv_i(run(T_i(lr)))  for i = 1..7;  out = acc * 0.125

24 x 40 is non-square and ragged against HAT's 16, DAT's 32 and NAFNet's 16 in both orientations (with reflect pads below the image
size), so the eight outputs differ and the mean is not the plain forward."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu


def torch_d4(x, code):
    if code & 1:
        x = x.flip(-1)
    if code & 2:
        x = x.flip(-2)
    return torch.rot90(x, code >> 2, dims=(-2, -1)).contiguous()


def torch_d4_undo(y, code):
    """The inverse of torch_d4(., code), spelled out step by step (independent of ops.d4_inverse_code)."""
    y = torch.rot90(y, -(code >> 2), dims=(-2, -1))
    if code & 2:
        y = y.flip(-2)
    if code & 1:
        y = y.flip(-1)
    return y.contiguous()


def torch_x8(run, lr, codes=range(8)):
    codes = list(codes)
    acc = None
    for c in codes:
        o = torch_d4_undo(run(torch_d4(lr, c)).clone(), c)
        acc = o if acc is None else acc + o
    return acc * torch.tensor(1.0 / len(codes), dtype=torch.float32, device=lr.device)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", params=["bf16x3", "bf16"])
def model(request, dev, synth_sd):
    from isr2_amd import ops
    from isr2_amd.model import FreqFusionHIP
    old = ops.gemm_mode()
    ops.set_gemm_mode(request.param)
    yield FreqFusionHIP(synth_sd, dev)
    ops.set_gemm_mode(old)


def _lr(shape, seed, dev):
    return torch.from_numpy(np.random.default_rng(seed).random(shape, dtype=np.float32)).to(dev)


@pytest.fixture(scope="module")
def eager(model, dev):
    """The eager ensembles the other tests compare against, computed once per mode: {name: (lr, result)}."""
    out = {}
    for name, shape, seed in (("24x40", (1, 3, 24, 40), 41), ("32x32", (1, 3, 32, 32), 42)):
        lr = _lr(shape, seed, dev)
        out[name] = (lr, model.self_ensemble(lr).clone())
    return out


def test_matches_torch_composition_and_is_not_a_no_op(model, eager):
    lr, got = eager["24x40"]
    assert tuple(got.shape) == (1, 3, 96, 160) and torch.isfinite(got).all()
    assert torch.equal(got, torch_x8(model, lr))
    assert not torch.equal(got, model(lr)), "the eight variants agree bit for bit: the ensemble is a no-op"
    lr, got = eager["32x32"]
    assert torch.equal(got, torch_x8(model, lr))


def test_codes_subset_order_and_out(model, dev, eager):
    lr, _ = eager["24x40"]
    codes = (5, 0, 13)
    out = torch.full((1, 3, 96, 160), float("nan"), device=dev)
    got = model.self_ensemble(lr, codes=codes, out=out)
    assert got is out and torch.equal(out, torch_x8(model, lr, codes))


def test_bad_codes_raise_before_any_launch(model, dev, eager):
    from isr2_amd import lib as L
    from isr2_amd.lib import FFError
    lr, _ = eager["24x40"]
    real, calls = L.load(), []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    L._lib = Spy()
    try:
        for codes in ((), (0, 16), (-1,), (0, 1, 0), (1, 10), (4, 15)):      # 10 = 1 and 15 = 4 as symmetries
            with pytest.raises(FFError):
                model.self_ensemble(lr, codes=codes)
        with pytest.raises(FFError):
            model.self_ensemble(lr[0])
        with pytest.raises(FFError):
            model.self_ensemble(lr, out=torch.empty(1, 3, 160, 96, device=dev))
    finally:
        L._lib = real
    assert not calls


def test_graph_replays_give_the_eager_bits(model, eager):
    for name in ("24x40", "32x32"):                                          # 24x40 replays two graphs, 24x40 and 40x24
        lr, ref = eager[name]
        assert torch.equal(model.self_ensemble(lr, run=model.graphed), ref), name
        assert torch.equal(model.self_ensemble(lr, run=model.graphed), ref), name     # pure replays, no capture in the loop


def test_two_lanes_are_bit_identical_to_the_sequential_loop(model, eager):
    lr, ref = eager["32x32"]
    got = model.self_ensemble(lr, run=model.graphed, run_async=model.graphed_async)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    got = model.self_ensemble(lr, run_async=model.graphed_async, codes=(3, 6, 1))          # an odd count drains both lanes in order
    torch.cuda.synchronize()
    assert torch.equal(got, torch_x8(model, lr, (3, 6, 1)))
    lr, ref = eager["24x40"]                                                  # a non-square input ignores the lanes
    seen = []

    def spy(t, lane):
        seen.append(lane)
        return model.graphed_async(t, lane)
    assert torch.equal(model.self_ensemble(lr, run=model.graphed, run_async=spy), ref) and not seen


def test_batch_of_two_is_two_single_images(model, dev, eager):
    a, ra = eager["24x40"]
    b = _lr((1, 3, 24, 40), 43, dev)
    got = model.self_ensemble(torch.cat([a, b]))
    assert tuple(got.shape) == (2, 3, 96, 160)
    assert torch.equal(got[0:1], ra) and torch.equal(got[1:2], model.self_ensemble(b))


def test_tile_route(model, dev):
    import models.team29_FreqFusion.io as plug
    lr = _lr((1, 3, 40, 56), 44, dev)

    def run(t):
        return plug._tiled_forward(model, t, 32, 8, 4, dev)
    assert torch.equal(model.self_ensemble(lr, run=run), torch_x8(run, lr))


def test_plugin_switch_writes_the_ensemble(tmp_path, model, dev, monkeypatch, capsys):
    import models.team29_FreqFusion.io as plug
    from isr2_amd import ops
    rng = np.random.default_rng(45)
    (tmp_path / "in").mkdir()
    imgs = {"a.png": rng.integers(0, 256, size=(24, 40, 3), dtype=np.uint8), "b.png": rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)}
    for name, u8 in imgs.items():
        Image.fromarray(u8).save(tmp_path / "in" / name)
    monkeypatch.setattr(plug, "_build_and_load", lambda model_dir, device, rank=0, world=1: model)
    monkeypatch.setenv("FF_ALLOW_SYNTH", "1")
    want = {}
    for name, u8 in imgs.items():
        lr = ops.u8_to_f32_image(torch.from_numpy(u8).to(dev))
        want[name] = ops.f32_to_u8_image(model.self_ensemble(lr)).cpu().numpy()
    plain = ops.f32_to_u8_image(model(ops.u8_to_f32_image(torch.from_numpy(imgs["a.png"]).to(dev)))).cpu().numpy()
    monkeypatch.setenv("FF_SELF_ENSEMBLE", "1")
    for threads in ("1", "0"):
        monkeypatch.setenv("FF_IO_THREADS", threads)
        dst = tmp_path / f"out{threads}"
        plug.main(model_dir="x.pth", input_path=str(tmp_path / "in"), output_path=str(dst), device=dev)
        assert "Self-ensemble: on" in capsys.readouterr().out
        assert sorted(os.listdir(dst)) == ["a.png", "b.png"]
        for name in imgs:
            assert np.array_equal(np.array(Image.open(dst / name).convert("RGB")), want[name]), (threads, name)
    # the switch off (0, empty, absent) is today's single pass
    for off in ("0", "", None):
        if off is None:
            monkeypatch.delenv("FF_SELF_ENSEMBLE")
        else:
            monkeypatch.setenv("FF_SELF_ENSEMBLE", off)
        dst = tmp_path / f"plain{off}"
        plug.main(model_dir="x.pth", input_path=str(tmp_path / "in"), output_path=str(dst), device=dev)
        assert "Self-ensemble" not in capsys.readouterr().out
        assert np.array_equal(np.array(Image.open(dst / "a.png").convert("RGB")), plain)
