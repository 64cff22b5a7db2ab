"""Host side of ff_hab_link (no GPU): the entry point is in the header and in the executor's generated dispatch, and everything the kernel
is not built for is refused with FF_ERR_ARG before any launch.  Every call here passes host addresses, so a call that slipped past the
checks could not run a kernel either -- and each refusal is identified by its own message, not only by its code."""
import ctypes
import os

import pytest

GOOD = dict(lda=192, ldx=192, ldc=192, scale_ld=180, B=2, H=32, W=32, ldxo=192, K=180, ht=12, nterms=1, io_bf16=3, ldo=192, o_off=0,
            rel_rows=31, rel_stride=48, wh=16, ww=16, sh=8, sw=8, use_mask=1, nheads=6, d=30, ldxn=192, out_bf16=1, xn_bf16=1)


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


def _call(L, p, ptrs=None, rpi=None, M=None, **kw):
    a = dict(GOOD, **kw)
    q = dict(att=p, x=p, c2=p, c2_scale=p, x_out=p, proj=p, bp=p, g2=p, b2n=p, mlp=p, b1=p, b2=p, att_out=p, g1=p, b1n=p, qkv=p, qb=p, rel=p, xn=p)
    q.update(ptrs or {})
    rpi = a["H"] * a["W"] if rpi is None else rpi
    M = a["B"] * rpi if M is None else M
    return L.ff_hab_link(q["att"], a["lda"], q["x"], a["ldx"], q["c2"], a["ldc"], q["c2_scale"], a["scale_ld"], a["B"], rpi, q["x_out"], a["ldxo"], M,
                         a["K"], a["ht"], q["proj"], q["bp"], q["g2"], q["b2n"], 1e-5, q["mlp"], q["b1"], q["b2"], a["nterms"], a["io_bf16"],
                         q["att_out"], a["ldo"], a["o_off"], q["g1"], q["b1n"], 1e-5, q["qkv"], q["qb"], q["rel"], a["rel_rows"], a["rel_stride"],
                         a["H"], a["W"], a["wh"], a["ww"], a["sh"], a["sw"], a["use_mask"], a["nheads"], a["d"], q["xn"], a["ldxn"],
                         a["out_bf16"], a["xn_bf16"], None)


def test_entry_point_is_declared_and_dispatched(L, tmp_path):
    from isr2_amd import build as B
    from isr2_amd.lib import parse_header
    protos = parse_header()
    assert "ff_hab_link" in protos
    ret, args = protos["ff_hab_link"]
    assert ret == "int" and args[-1] == "void*" and len(args) == 50
    assert L.ff_abi_version() == 7                                      # an additive entry point
    gen = os.path.join(str(tmp_path), "ff_dispatch_gen.h")
    B.gen_dispatch(gen)                                                 # what build() generates for csrc/ff_executor.hip
    txt = open(gen).read()
    assert '"ff_hab_link"' in txt and "return ff_hab_link(" in txt


REFUSALS = [
    ("split products", dict(nterms=3), b"plain bf16 only"),
    ("window 8x32", dict(wh=8, ww=32), b"16x16"),
    ("window 32x8", dict(wh=32, ww=8), b"16x16"),
    ("head dim 32", dict(d=32), b"six heads of dim 30"),
    ("five heads", dict(nheads=5), b"six heads of dim 30"),
    ("K 176", dict(K=176), b"K must be 180"),
    ("H 40", dict(H=40), b"multiples of 16"),
    ("W 24", dict(W=24), b"multiples of 16"),
    ("fp32 att", dict(io_bf16=2), b"bf16 rows"),
    ("fp32 c2", dict(io_bf16=1), b"bf16 rows"),
    ("fp32 att out", dict(out_bf16=0), b"bf16 rows"),
    ("fp32 xn", dict(xn_bf16=0), b"bf16 rows"),
    ("att pitch 180", dict(lda=180), b"att rows must be 16-byte aligned"),
    ("x pitch 182", dict(ldx=182), b"x / x_out rows"),
    ("x_out pitch 190", dict(ldxo=190), b"x / x_out rows"),
    ("c2 pitch 181", dict(ldc=181), b"c2 rows 8-byte aligned"),
    ("gate pitch 182", dict(scale_ld=182), b"gate rows"),
    ("xn pitch 180", dict(ldxn=180), b"xn rows"),
    ("att out pitch 181", dict(ldo=181), b"att_out rows"),
    ("13 hidden tiles", dict(ht=13), b"hidden tiles"),
    ("2^31 row offsets", dict(B=2731, H=64, W=64), b"2^31"),           # (the bound itself: test_row_offset_bound_is_exact)
]


@pytest.mark.parametrize("what,kw,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_before_any_launch(L, ptr, what, kw, msg):
    assert _call(L, ptr, **kw) == 1, what                               # FF_ERR_ARG
    err = L.ff_last_error()
    assert b"ff_hab_link" in err and msg in err, err


def test_row_offset_bound_is_exact(L, ptr):
    # 64 x 64 images at pitch 192: B * 4096 * 192 < 2^31  <=>  B <= 2730; the call below passes every argument check but this one
    assert 2730 * 4096 * 192 < 2 ** 31 <= 2731 * 4096 * 192
    assert _call(L, ptr, B=2731, H=64, W=64) == 1 and b"2^31" in L.ff_last_error()


@pytest.mark.parametrize("name", ["c2", "c2_scale"])
def test_missing_conv_branch_or_gate_is_refused(L, ptr, name):
    assert _call(L, ptr, ptrs={name: None}) == 1
    assert b"c2 and the gate are required" in L.ff_last_error()


@pytest.mark.parametrize("name", ["att", "x", "x_out", "proj", "mlp", "att_out", "qkv", "rel", "xn", "g1", "g2"])
def test_null_pointers_are_refused(L, ptr, name):
    assert _call(L, ptr, ptrs={name: None}) == 1
    assert b"ff_hab_link: null pointer" in L.ff_last_error()


@pytest.mark.parametrize("name,msg", [("att", b"att rows"), ("x", b"x / x_out rows"), ("x_out", b"x / x_out rows"), ("c2_scale", b"gate rows"),
                                      ("xn", b"xn rows"), ("qkv", b"weights"), ("rel", b"weights"), ("b2", b"weights")])
def test_misaligned_addresses_are_refused(L, ptr, name, msg):
    assert _call(L, ptr, ptrs={name: ptr + 4}) == 1
    err = L.ff_last_error()
    assert b"ff_hab_link" in err and msg in err, err


def test_geometry_must_agree(L, ptr):
    assert _call(L, ptr, rpi=512) == 1 and b"rows_per_image" in L.ff_last_error()
    assert _call(L, ptr, M=1024) == 1 and b"rows_per_image" in L.ff_last_error()
    assert _call(L, ptr, use_mask=1, sh=0, sw=0) == 1 and b"mask needs a shift" in L.ff_last_error()
    assert _call(L, ptr, sh=16) == 1 and b"bad shift" in L.ff_last_error()
    assert _call(L, ptr, rel_stride=64) == 1 and b"bias table" in L.ff_last_error()
