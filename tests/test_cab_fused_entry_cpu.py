"""Host side of ff_cab_fused (no GPU): the entry point is in the header and in the executor's generated dispatch, and everything the kernel
is not built for is refused with FF_ERR_ARG before any launch.  Every call here passes host addresses, so a call that slipped past the
checks could not run a kernel either -- and each refusal is identified by its own message, not only by its code."""
import ctypes
import os

import pytest

GOOD = dict(ldi=192, ldo=192, B=2, H=32, W=32, Cin=180, Cmid=60, Cout=180, nterms=1, io_bf16=3)


@pytest.fixture(scope="module")
def L():
    from isr2_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def ptr():
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    yield p
    del buf


def _call(L, p, ptrs=None, w1_bytes=None, w2_bytes=None, **kw):
    a = dict(GOOD, **kw)
    q = dict(xn=p, w1=p, b1=p, w2=p, b2=p, c2=p + 64, part=p)
    q.update(ptrs or {})
    w1_bytes = L.ff_conv3x3_halo_weight_bytes(60, 180, 64, 1) if w1_bytes is None else w1_bytes
    w2_bytes = L.ff_conv3x3_halo_weight_bytes(180, 60, 192, 1) if w2_bytes is None else w2_bytes
    return L.ff_cab_fused(q["xn"], a["ldi"], q["w1"], w1_bytes, q["b1"], q["w2"], w2_bytes, q["b2"], q["c2"], a["ldo"], q["part"],
                          a["B"], a["H"], a["W"], a["Cin"], a["Cmid"], a["Cout"], a["nterms"], a["io_bf16"], None)


def test_entry_point_is_declared_and_dispatched(L, tmp_path):
    from isr2_amd import build as B
    from isr2_amd.lib import parse_header
    protos = parse_header()
    assert "ff_cab_fused" in protos
    ret, args = protos["ff_cab_fused"]
    assert ret == "int" and args[-1] == "void*" and len(args) == 20
    assert L.ff_abi_version() == 7                                      # an additive entry point
    assert "cab_fused.hip" in B.SOURCES
    gen = os.path.join(str(tmp_path), "ff_dispatch_gen.h")
    B.gen_dispatch(gen)                                                 # what build() generates for csrc/ff_executor.hip
    txt = open(gen).read()
    assert '"ff_cab_fused"' in txt and "return ff_cab_fused(" in txt


def test_weight_image_sizes_are_the_halo_images(L):
    # 3 chunks x 9 taps x (64 rows x 144 B) and 9 taps x 2 halves x (192 rows x 80 B): the tiles the kernel's two rings stream
    assert L.ff_conv3x3_halo_weight_bytes(60, 180, 64, 1) == 27 * 9216
    assert L.ff_conv3x3_halo_weight_bytes(180, 60, 192, 1) == 18 * 15360


REFUSALS = [
    ("split products", dict(nterms=3), b"plain bf16 only"),
    ("fp32 xn", dict(io_bf16=2), b"bf16 rows"),
    ("fp32 c2", dict(io_bf16=1), b"bf16 rows"),
    ("fp32 rows", dict(io_bf16=0), b"bf16 rows"),
    ("Cin 176", dict(Cin=176), b"180 -> 60 -> 180"),
    ("Cmid 64", dict(Cmid=64), b"180 -> 60 -> 180"),
    ("Cout 192", dict(Cout=192), b"180 -> 60 -> 180"),
    ("H 40", dict(H=40), b"multiples of 16"),
    ("W 24", dict(W=24, H=64), b"multiples of 16"),
    ("16 x 16", dict(H=16, W=16), b"at least 1024"),
    ("16 x 48", dict(H=16, W=48), b"at least 1024"),
    ("xn pitch 180", dict(ldi=180), b"xn rows must be 16-byte aligned"),
    ("xn pitch 176", dict(ldi=176), b"xn rows must be 16-byte aligned"),
    ("c2 pitch 182", dict(ldo=182), b"c2 rows must be 8-byte aligned"),
    ("c2 pitch 176", dict(ldo=176), b"c2 rows must be 8-byte aligned"),
    ("2^31 row offsets", dict(B=2731, H=64, W=64), b"2^31"),            # (the bound itself: test_row_offset_bound_is_exact)
]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_launch(L, ptr, what, kw, msg):
    assert _call(L, ptr, **kw) == 1, what                               # FF_ERR_ARG
    err = L.ff_last_error()
    assert b"ff_cab_fused" in err and msg in err, err


def test_row_offset_bound_is_exact(L, ptr):
    # 64 x 64 images at pitch 192: B * 4096 * 192 < 2^31  <=>  B <= 2730; the call below passes every argument check but this one
    assert 2730 * 4096 * 192 < 2 ** 31 <= 2731 * 4096 * 192
    assert _call(L, ptr, B=2731, H=64, W=64) == 1 and b"2^31" in L.ff_last_error()
    assert _call(L, ptr, B=2800, H=64, W=64, ldi=184) == 1 and b"2^31" in L.ff_last_error()      # the wider of the two pitches counts


@pytest.mark.parametrize("which,shape,bn,msg", [("w1_bytes", (60, 180), 64, b"conv1's weight image"), ("w2_bytes", (180, 60), 192, b"conv2's weight image")])
def test_weight_image_of_another_size_is_refused(L, ptr, which, shape, bn, msg):
    # the other packings of the same weight: split products (nterms 3), another tile width, the other convolution's image; and no image
    good = L.ff_conv3x3_halo_weight_bytes(*shape, bn, 1)
    others = [L.ff_conv3x3_halo_weight_bytes(*shape, bn, 3), L.ff_conv3x3_halo_weight_bytes(*shape, 32, 1),
              L.ff_conv3x3_halo_weight_bytes(*shape, 128, 1), L.ff_conv3x3_halo_weight_bytes(*shape[::-1], 256 - bn, 1), good - 1024, 0, -1]
    others = [v for v in others if v != good]                           # (a few packings of other shapes happen to have the same size)
    assert len(others) >= 5
    for other in others:
        assert _call(L, ptr, **{which: other}) == 1
        err = L.ff_last_error()
        assert b"ff_cab_fused" in err and msg in err, err


def test_aliasing_is_refused(L, ptr):
    assert _call(L, ptr, ptrs={"c2": ptr}) == 1
    assert b"c2 must not alias xn" in L.ff_last_error()


@pytest.mark.parametrize("name", ["xn", "w1", "b1", "w2", "b2", "c2", "part"])
def test_null_pointers_are_refused(L, ptr, name):
    assert _call(L, ptr, ptrs={name: None}) == 1
    assert b"ff_cab_fused: null pointer" in L.ff_last_error()


@pytest.mark.parametrize("name,msg", [("xn", b"xn rows"), ("c2", b"c2 rows"), ("w1", b"weight images"), ("w2", b"weight images")])
def test_misaligned_addresses_are_refused(L, ptr, name, msg):
    assert _call(L, ptr, ptrs={name: ptr + 4}) == 1
    err = L.ff_last_error()
    assert b"ff_cab_fused" in err and msg in err, err
