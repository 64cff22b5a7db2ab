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


def _bit_patterns(shape, seed, dev):
    """Seeded random 32-bit patterns as int32 (every exponent field: denormals, infinities and NaNs of either kind occur), with
    -0.0, +-inf, the smallest denormal, a signalling and a payload-carrying quiet NaN planted at the front."""
    bits = np.random.default_rng(seed).integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)
    special = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7F800001, 0x7FC12345, 0xFFA00000],
                       dtype=np.uint32).view(np.int32)
    bits.reshape(-1)[:special.size] = special
    return torch.from_numpy(bits).to(dev)


def test_d4_nchw_is_a_pure_copy_and_d4_rect_agrees(dev):
    """ops.d4_nchw moves bits: no multiply and no add may touch a value, so denormals, negative zero, infinities and NaN payloads
    (signalling ones included) arrive unchanged -- compared as int32 against torch's flip / rot90 of the int32 view.  65 x 65 is
    ragged on both axes and takes the dword rows and the transpose; 7 x 12 takes the float4 rows in a tile narrower than 64.
    ops.d4_rect with scale 1 is the same permutation through the emit form, t * 1: exact for every value but a signalling NaN,
    which the multiply quiets (its contract, not the copy's) -- so the same bit patterns with the signalling NaNs made quiet
    (bit 22 set) must come out of both bit for bit; a flush of denormals, a lost sign of zero or a stray add would show.
    65 x 65 again, and 130 x 64 (three tiles down, float4 rows)."""
    from isr2_amd import ops
    for shape, codes in (((2, 3, 65, 65), range(16)), ((1, 1, 7, 12), [c for c in range(16) if not c & 4])):
        xi = _bit_patterns(shape, 21, dev)
        for c in codes:
            got = ops.d4_nchw(xi.view(torch.float32), [c] * shape[0])
            assert torch.equal(got.view(torch.int32), torch_d4(xi, c)), (shape, c)
    for shape, codes in (((2, 3, 65, 65), range(16)), ((1, 2, 130, 64), [c for c in range(16) if not c & 4])):
        xi = _bit_patterns(shape, 22, dev)
        snan = ((xi & 0x7F800000) == 0x7F800000) & ((xi & 0x007FFFFF) != 0) & ((xi & 0x00400000) == 0)
        assert snan.any()
        x = torch.where(snan, xi | 0x00400000, xi).view(torch.float32)
        for c in codes:
            a, b = ops.d4_rect(x, c), ops.d4_nchw(x, [c] * shape[0])
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (shape, c)
