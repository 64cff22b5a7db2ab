"""ops.cab_fused (csrc/cab_fused.hip): HAT's CAB convolutions in one launch against the two launches it replaces, bit for bit -- torch.equal
on c2 (bf16), on the pool partial rows and on the gate ops.vec_mlp makes of them.  The reference is computed in the same test by the
per-launch route's own calls (ops.conv2d + ops.conv2d(want_pool="partials") + ops.vec_mlp), never by the code under test; the fused kernel
issues the same MFMAs in the same order, so there is no tolerance.

Shapes, the smallest where each thing can go wrong: 32 x 32 is four 16 x 16 tiles, every one on two image borders (c1 positions outside
the image must be zero, not conv1 of a zero-padded input); 48 x 48 has one interior tile with halos from all eight neighbours; 32 x 64 and
64 x 32 tell the tile remap's rows from its columns; B = 2 and 3 group the partial rows by image, and image b must equal its own B = 1 call.
Both biases are non-zero (gelu(0) = 0 would hide a missing zero of the out-of-image c1 positions) and one case draws conv1's around +1."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

C, CM = 180, 60


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


class _Mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from isr2_amd import ops
        self.prev = ops.gemm_mode()
        ops.set_gemm_mode(self.mode)
        return ops

    def __exit__(self, *exc):
        from isr2_amd import ops
        ops.set_gemm_mode(self.prev)


def _weights(dev, bias1_mean):
    # packed tap-major weights [Cout, 9 * Cin]; conv1's pre-activation has unit scale (GELU in its curved range)
    cab0 = (rnd(CM, 9 * C, dev=dev, seed=2001, scale=1.0 / math.sqrt(9 * C)).contiguous(),
            (rnd(CM, dev=dev, seed=2002, scale=0.3) + bias1_mean).contiguous())
    cab2 = (rnd(C, 9 * CM, dev=dev, seed=2003, scale=1.0 / math.sqrt(9 * CM)).contiguous(),
            (rnd(C, dev=dev, seed=2004, scale=0.2) + 0.05).contiguous())
    ca1 = (rnd(6, C, dev=dev, seed=2005, scale=1.0 / math.sqrt(C)).contiguous(), rnd(6, dev=dev, seed=2006, scale=0.1).contiguous())
    ca2 = (rnd(C, 6, dev=dev, seed=2007, scale=0.4).contiguous(), rnd(C, dev=dev, seed=2008, scale=0.1).contiguous())
    assert cab0[1].abs().min() > 0 and cab2[1].abs().min() > 0
    return dict(cab0=cab0, cab2=cab2, ca1=ca1, ca2=ca2)


@pytest.fixture(scope="module")
def weights(dev):
    return _weights(dev, 0.1)


@pytest.fixture(scope="module")
def weights_bias1(dev):
    return _weights(dev, 1.0)


def _xn(B, H, W, dev, seed, garbage=False):
    from isr2_amd import ops
    t = ops.empty_rows_bf16((B, H, W, C), dev)
    assert t.stride(-2) == 192
    if garbage:                                              # columns 180..191 of every row: not the tensor's, must not reach a result
        base = torch.empty(0, dtype=torch.bfloat16, device=dev).set_(t.untyped_storage(), 0, (B * H * W, 192))
        base[:, 180:186] = float("nan")
        base[:, 186:] = 3.0e38
    t.copy_(rnd(B, H, W, C, dev=dev, seed=seed))
    return t


def _gate(ops, pp, w):
    return ops.vec_mlp(pp, *w["ca1"], "relu", *w["ca2"], "sigmoid", post=0.01)


def _reference(ops, xn, w):
    c1 = ops.conv2d(xn, *w["cab0"], ksize=(3, 3), pad=(1, 1), act="gelu", out_bf16=True, per_image=True)
    c2, pp = ops.conv2d(c1, *w["cab2"], ksize=(3, 3), pad=(1, 1), want_pool="partials", out_bf16=True)
    return c2, pp, _gate(ops, pp, w)


def _check(ops, xn, w, tag=""):
    c2_ref, pp_ref, gate_ref = _reference(ops, xn, w)
    c2, pp = ops.cab_fused(xn, w["cab0"], w["cab2"])
    gate = _gate(ops, pp, w)
    torch.cuda.synchronize()
    assert c2.dtype == torch.bfloat16 and tuple(c2.shape) == tuple(xn.shape) and c2.stride(-2) == c2_ref.stride(-2)
    assert torch.isfinite(c2_ref.float()).all() and torch.isfinite(pp_ref.part).all()
    assert (pp.part.shape, pp.C, pp.inv_count, pp.images) == (pp_ref.part.shape, pp_ref.C, pp_ref.inv_count, pp_ref.images)
    assert torch.equal(c2, c2_ref), f"{tag}c2: max diff {(c2.float() - c2_ref.float()).abs().max().item():.3e}"
    assert torch.equal(pp.part, pp_ref.part), f"{tag}partial rows: max diff {(pp.part - pp_ref.part).abs().max().item():.3e}"
    assert torch.equal(gate, gate_ref), f"{tag}gate"
    return c2, pp


@pytest.mark.parametrize("H,W", [(32, 32), (48, 48), (32, 64), (64, 32)])
def test_cab_fused_equals_the_two_launches(dev, weights, H, W):
    with _Mode("bf16") as ops:
        _check(ops, _xn(1, H, W, dev, 2010), weights)


def test_conv1_bias_around_one(dev, weights_bias1):
    # gelu(1) = 0.84: a c1 position outside the image that held conv1 of the zero padding (or its bias alone) instead of zero shows in every border pixel
    with _Mode("bf16") as ops:
        c2, _ = _check(ops, _xn(1, 32, 32, dev, 2011), weights_bias1)
        zero_in = ops.empty_rows_bf16((1, 32, 32, C), dev)
        zero_in.zero_()
        _check(ops, zero_in, weights_bias1, "zero input: ")


def test_pad_columns_are_not_read(dev, weights):
    with _Mode("bf16") as ops:
        clean, dirty = _xn(1, 32, 32, dev, 2012), _xn(1, 32, 32, dev, 2012, garbage=True)
        assert torch.equal(clean, dirty)
        c2, pp = _check(ops, dirty, weights)
        c2_clean, pp_clean = ops.cab_fused(clean, weights["cab0"], weights["cab2"])
        assert torch.equal(c2, c2_clean) and torch.equal(pp.part, pp_clean.part)


@pytest.mark.parametrize("B", [2, 3])
def test_batch_is_one_launch_with_every_image_its_own(dev, weights, B):
    with _Mode("bf16") as ops:
        xn = _xn(B, 32, 32, dev, 2013)
        with ops.profile() as prof:
            c2, pp = ops.cab_fused(xn, weights["cab0"], weights["cab2"])
        assert [r[0] for r in prof.records()] == ["cab_fused"]
        _check(ops, xn, weights)
        assert pp.images == B and pp.part.shape[0] == 4 * B
        for b in range(B):
            one = ops.empty_rows_bf16((1, 32, 32, C), dev)
            one.copy_(xn[b:b + 1])
            c2_1, pp_1 = ops.cab_fused(one, weights["cab0"], weights["cab2"])
            assert torch.equal(c2[b:b + 1], c2_1), f"image {b}"
            assert torch.equal(pp.part[4 * b:4 * b + 4], pp_1.part), f"image {b}: partial rows"
        assert not torch.equal(c2[0], c2[1])


def test_second_call_into_the_same_buffer(dev, weights):
    # the launch keeps no state between calls: a second call over the first one's output gives the same c2 and partial rows
    with _Mode("bf16") as ops:
        xn = _xn(2, 32, 32, dev, 2014)
        out = ops.empty_rows_bf16((2, 32, 32, C), dev)
        c2a, ppa = ops.cab_fused(xn, weights["cab0"], weights["cab2"], out=out)
        first, first_part = c2a.clone(), ppa.part.clone()
        c2b, ppb = ops.cab_fused(xn, weights["cab0"], weights["cab2"], out=out)
        torch.cuda.synchronize()
        assert c2b.data_ptr() == out.data_ptr()
        assert torch.equal(c2b, first) and torch.equal(ppb.part, first_part)
        assert torch.equal(_gate(ops, ppb, weights), _gate(ops, ppa, weights))


def test_under_a_captured_graph(dev, weights):
    with _Mode("bf16") as ops:
        xn = _xn(2, 32, 32, dev, 2015)
        c2_ref, pp_ref, gate_ref = _reference(ops, xn, weights)
        ops.cab_fused(xn, weights["cab0"], weights["cab2"])                 # weight images and the kernel's LDS attribute exist before the capture
        torch.cuda.synchronize()
        s = torch.cuda.Stream(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                c2, pp = ops.cab_fused(xn, weights["cab0"], weights["cab2"])
                gate = _gate(ops, pp, weights)
        for _ in range(2):
            c2.zero_()
            pp.part.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(c2, c2_ref) and torch.equal(pp.part, pp_ref.part) and torch.equal(gate, gate_ref)


def test_predicate_takes_only_what_the_kernel_takes(dev):
    # what HatHIP routes by: anything the entry point would refuse keeps the two launches instead of raising
    with _Mode("bf16") as ops:
        good = _xn(1, 32, 32, dev, 2017)
        assert ops.cab_fused_ok(good)
        assert not ops.cab_fused_ok(good.float())                                               # fp32 rows
        assert not ops.cab_fused_ok(torch.empty((1, 32, 32, C), device=dev, dtype=torch.bfloat16))   # pitch 180: rows not 16-byte aligned
        assert not ops.cab_fused_ok(_xn(1, 32, 48, dev, 2017)[:, :, 1:33])                      # (a column window: rows do not collapse to one pitch)
        assert not ops.cab_fused_ok(_xn(1, 16, 16, dev, 2017)) and not ops.cab_fused_ok(_xn(1, 40, 32, dev, 2017))
    with _Mode("bf16x3") as ops:
        assert not ops.cab_fused_ok(good)


def test_needs_plain_bf16(dev, weights):
    from isr2_amd.lib import FFError
    with _Mode("bf16x3") as ops:
        with pytest.raises(FFError):
            ops.cab_fused(_xn(1, 32, 32, dev, 2016), weights["cab0"], weights["cab2"])


# ---- HatHIP.group ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hat(dev, synth_sd):
    from isr2_amd.experts import HatHIP
    return HatHIP(synth_sd, dev)


def _rows(B, H, W, dev, seed):
    from isr2_amd import ops
    t = ops.empty_rows((B, H, W, C), dev)
    t.copy_(rnd(B, H, W, C, dev=dev, seed=seed))
    return t


@pytest.mark.parametrize("B", [1, 2])
def test_group_equals_the_per_launch_route(dev, hat, B):
    with _Mode("bf16") as ops:
        x = _rows(B, 32, 32, dev, 2020)
        hat._cab_fused = lambda xn: False                                # the instance's predicate off: conv2d + conv2d as before
        try:
            with ops.profile() as prof:
                want = hat.group(x, 0)
            old = [r[0] for r in prof.records()]
        finally:
            del hat._cab_fused
        with ops.profile() as prof:
            got = hat.group(x, 0)
        new = [r[0] for r in prof.records()]
        assert "cab_fused" not in old and new.count("cab_fused") == 6 and len(old) - len(new) == 6, (old, new)
        assert torch.isfinite(want).all()
        assert torch.equal(got, want), f"max diff {(got - want).abs().max().item():.3e}"


def test_group_keeps_its_launches_in_bf16x3(dev, hat):
    with _Mode("bf16x3") as ops:
        x = _rows(1, 32, 32, dev, 2021)
        with ops.profile() as prof:
            hat.group(x, 0)
        assert "cab_fused" not in [r[0] for r in prof.records()]
