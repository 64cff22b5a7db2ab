"""ff_d4_rect_nchw (ops.d4_rect): one symmetry of the square on rectangular planes, with fused accumulation -- bit for bit against
torch's flip / rot90 composition.  The shapes are the smallest that reach every path of the kernel: less than one 64 x 64 tile with
W % 4 != 0 (dword rows), ragged on both axes, exactly one tile, several tiles with 16-byte rows and one ragged axis, the other axis
ragged, and a contiguous view that starts one float into its storage (unaligned base: dword rows although W % 4 == 0)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 5, 7), (2, 3, 37, 53), (1, 2, 64, 64), (1, 3, 130, 68), (1, 1, 64, 200)]


def torch_d4(x, code):
    if code & 1:
        x = x.flip(-1)
    if code & 2:
        x = x.flip(-2)
    return torch.rot90(x, code >> 2, dims=(-2, -1)).contiguous()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rand(shape, seed, dev):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)).to(dev)


def _unaligned(shape, seed, dev):
    """A contiguous tensor of `shape` whose first element sits one float into a 16-byte aligned allocation."""
    n = int(np.prod(shape))
    buf = torch.empty(n + 1, device=dev, dtype=torch.float32)
    x = buf[1:].view(shape)
    x.copy_(_rand(shape, seed, dev))
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    return x


@pytest.mark.parametrize("shape", SHAPES + ["unaligned"], ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_every_code_matches_torch(dev, shape):
    from isr2_amd import ops
    x = _unaligned((1, 2, 36, 68), 3, dev) if shape == "unaligned" else _rand(shape, 1, dev)
    for c in range(16):
        want = torch_d4(x, c)
        got = ops.d4_rect(x, c)
        assert got.shape == want.shape and got.is_contiguous() and torch.equal(got, want), (shape, c)
    if shape == "unaligned":                                      # an unaligned destination as well
        for c in (3, 6, 9):
            out = _unaligned(tuple(torch_d4(x, c).shape), 4, dev)
            assert ops.d4_rect(x, c, out=out) is out and torch.equal(out, torch_d4(x, c)), c


@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (1, 3, 130, 68), "unaligned"], ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_accumulate_rounds_the_add_then_the_multiply(dev, shape, scale):
    from isr2_amd import ops
    x = _unaligned((1, 2, 36, 68), 3, dev) if shape == "unaligned" else _rand(shape, 1, dev)
    for c in range(16):
        t = torch_d4(x, c)
        seed = _rand(tuple(t.shape), 100 + c, dev)
        dst = seed.clone()
        got = ops.d4_rect(x, c, out=dst, accum=True, scale=scale)
        assert got is dst
        assert torch.equal(dst, (seed + t) * scale), (shape, c, scale)
        assert torch.equal(ops.d4_rect(x, c, scale=scale), t * scale), (shape, c, scale)
    # scale = 1/3 is not a power of two: the product of the ROUNDED sum, never a fused multiply-add of the parts
    third = float(np.float32(1.0 / 3.0))
    t = torch_d4(x, 5)
    seed = _rand(tuple(t.shape), 7, dev)
    dst = seed.clone()
    ops.d4_rect(x, 5, out=dst, accum=True, scale=third)
    assert torch.equal(dst, (seed + t) * torch.tensor(third, device=dev))


def test_inverse_code_round_trip(dev):
    from isr2_amd import ops
    x = _rand((2, 3, 37, 53), 11, dev)
    for c in range(16):
        back = ops.d4_rect(ops.d4_rect(x, c), ops.d4_inverse_code(c))
        assert back.shape == x.shape and torch.equal(back, x), c


def test_host_checks_refuse_before_any_launch(dev):
    from isr2_amd import lib as L
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    x = _rand((1, 3, 6, 10), 2, dev)
    real, calls = L.load(), []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    bad = [
        lambda: ops.d4_rect(x, 16),
        lambda: ops.d4_rect(x, -1),
        lambda: ops.d4_rect(x.cpu(), 0),
        lambda: ops.d4_rect(x.double(), 0),
        lambda: ops.d4_rect(x[0], 0),
        lambda: ops.d4_rect(x[..., ::2], 0),                                   # not contiguous
        lambda: ops.d4_rect(x, 4, out=torch.empty_like(x)),                    # odd k: out must be [1,3,10,6]
        lambda: ops.d4_rect(x, 0, out=torch.empty(1, 3, 10, 6, device=dev)),
        lambda: ops.d4_rect(x, 0, out=x),
        lambda: ops.d4_rect(x, 0, accum=True),                                 # nothing to accumulate into
        lambda: ops.d4_rect(x, 0, out=torch.empty(1, 3, 6, 10, device=dev, dtype=torch.float64)),
    ]
    L._lib = Spy()
    try:
        for f in bad:
            with pytest.raises(FFError):
                f()
        # ops.d4_nchw keeps refusing odd quarter turns on non-square planes (the training loader relies on one shape per batch)
        with pytest.raises(FFError):
            ops.d4_nchw(x, [4])
    finally:
        L._lib = real
    assert "ff_d4_rect_nchw" not in calls and "ff_d4_nchw" not in calls
