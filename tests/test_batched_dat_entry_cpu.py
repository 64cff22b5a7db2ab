"""Host side of DAT's per-image entry points (no GPU): the four new symbols, the partial-row and workspace helpers, and the geometry
checks that refuse a launch.  Every refusal asked for here is the entry point's FIRST check, made with host addresses before anything
touches the device: were a check to regress, these calls still could not reach a launch."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from isr2_amd import lib
    return lib.load()


_BUF = (ctypes.c_float * 128)()                                  # host memory: never dereferenced, only its (aligned) address is passed


@pytest.fixture(scope="module")
def p():
    a = ctypes.addressof(_BUF)
    return a + (-a) % 16


def _refused(L, status, name):
    assert status == 1, name                                     # FF_ERR_ARG
    assert name.encode() in L.ff_last_error(), L.ff_last_error()


# (B, rows per image, M): no image, half a workgroup, one row short of a workgroup, an image and a half, M that is not B images
BAD_GEOMETRY = [(0, 256, 0), (-1, 256, 256), (2, 128, 256), (2, 255, 510), (2, 384, 768), (2, 0, 0), (2, 256, 511), (2, 256, 768), (3, 256, 512)]


def test_new_symbols_are_declared_and_exported(L):
    from isr2_amd.lib import parse_header
    protos = parse_header()
    for name in ("ff_chan_attn_finish_images", "ff_conv2d_bf16s_wimages", "ff_token_linear_gated_images", "ff_pool_partials_images",
                 "ff_pool_partials_images_rows", "ff_chan_qkv_images_workspace"):
        assert name in protos, name
        assert getattr(L, name) is not None
    assert L.ff_abi_version() == 7                               # additive entry points: the version stays


@pytest.mark.parametrize("P", [256, 2304, 6400, 65536, 1024 * 1024])
def test_pool_partials_images_rows_is_b_times_one_image(L, P):
    one = L.ff_pool_partial_rows(P)
    assert one > 0
    for B in (1, 2, 5, 16):
        assert L.ff_pool_partials_images_rows(B, P) == B * one
    for B in (0, -2, 70000):
        assert L.ff_pool_partials_images_rows(B, P) == -1
    assert L.ff_pool_partials_images_rows(2, P - 1) == -1 and L.ff_pool_partials_images_rows(2, 0) == -1


@pytest.mark.parametrize("rows", [256, 768, 2304, 6400, 65536])
def test_chan_qkv_images_workspace_is_b_times_one_image(L, rows):
    one = L.ff_chan_qkv_workspace(rows)
    nblk = rows // 256
    assert one >= (nblk + 1) * 5760
    for B in (1, 2, 5, 16):
        ws = L.ff_chan_qkv_images_workspace(B, rows)
        assert ws == B * one
        assert ws >= (B * nblk + B) * 5760                       # the partials of every image, then one G block per image
    for B in (0, -1, 70000):
        assert L.ff_chan_qkv_images_workspace(B, rows) == -1
    assert L.ff_chan_qkv_images_workspace(2, rows + 1) == -1 and L.ff_chan_qkv_images_workspace(2, 0) == -1


def test_chan_attn_finish_images_refusals(L, p):
    name = "ff_chan_attn_finish_images"
    for B, rpi, _ in BAD_GEOMETRY:
        if B >= 1 and rpi > 0 and rpi % 256 == 0:
            continue                                             # (this entry takes no M: B and the rows per image are its geometry)
        _refused(L, L.ff_chan_attn_finish_images(p, 1 << 40, B, rpi, p, p, None), name)
    _refused(L, L.ff_chan_attn_finish_images(p, 1 << 40, 70000, 256, p, p, None), name)
    _refused(L, L.ff_chan_attn_finish_images(None, 1 << 40, 2, 256, p, p, None), name)
    _refused(L, L.ff_chan_attn_finish_images(p, 1 << 40, 2, 256, None, p, None), name)
    _refused(L, L.ff_chan_attn_finish_images(p, 1 << 40, 2, 256, p, None, None), name)
    _refused(L, L.ff_chan_attn_finish_images(p, 2 * 2 * 5760 - 1, 2, 256, p, p, None), name)      # workspace: B * (nblk + 1) blocks


def test_conv2d_bf16s_wimages_refusals(L, p):
    name = "ff_conv2d_bf16s_wimages"

    def call(inp=p, hi=p, lo=p, out=p, M=512, B=2, rpi=256, nterms=3, Cin=180, Kp=192):
        return L.ff_conv2d_bf16s_wimages(inp, 192, hi, lo, Kp, Kp, B, rpi, None, None, None, 0, out, 192, M, Cin, 180, nterms, 0, None)

    for B, rpi, M in BAD_GEOMETRY:
        # the geometry check comes first: null pointers behind it are never looked at
        _refused(L, call(B=B, rpi=rpi, M=M), name)
        assert b"rows_per_image" in L.ff_last_error()
        _refused(L, call(B=B, rpi=rpi, M=M, inp=None, hi=None, out=None), name)
        assert b"rows_per_image" in L.ff_last_error()
    for kw in (dict(inp=None), dict(hi=None), dict(out=None), dict(lo=None), dict(nterms=0), dict(Cin=178), dict(Kp=160)):
        _refused(L, call(**kw), name)


def test_token_linear_gated_images_refusals(L, p):
    name = "ff_token_linear_gated_images"

    def call(x=p, x2=p, cm=p, out=p, w=p, M=512, B=2, rpi=256, nterms=3, K=180):
        return L.ff_token_linear_gated_images(x, 192, x2, 192, cm, B, rpi, p, p, 0.1, out, 192, M, K, 180, 6, w, p, None, 0, nterms, None)

    for B, rpi, M in BAD_GEOMETRY:
        _refused(L, call(B=B, rpi=rpi, M=M), name)
        assert b"rows_per_image" in L.ff_last_error()
        _refused(L, call(B=B, rpi=rpi, M=M, x=None, cm=None, out=None), name)
        assert b"rows_per_image" in L.ff_last_error()
    _refused(L, call(B=70000, M=70000 * 256), name)
    for kw in (dict(x=None), dict(x2=None), dict(cm=None), dict(out=None), dict(w=None), dict(nterms=2), dict(K=200), dict(cm=p + 4)):
        _refused(L, call(**kw), name)


def test_pool_partials_images_refusals(L, p):
    name = "ff_pool_partials_images"
    for B, P, _ in BAD_GEOMETRY:
        if B >= 1 and P > 0 and P % 256 == 0:
            continue                                             # (no M here either: B images of P pixels)
        _refused(L, L.ff_pool_partials_images(p, 192, B, P, 180, p, 1 << 40, None), name)
        _refused(L, L.ff_pool_partials_images(None, 192, B, P, 180, None, 1 << 40, None), name)
        assert b"multiple of 256" in L.ff_last_error()
    _refused(L, L.ff_pool_partials_images(p, 192, 70000, 256, 180, p, 1 << 40, None), name)
    _refused(L, L.ff_pool_partials_images(None, 192, 2, 256, 180, p, 1 << 40, None), name)
    _refused(L, L.ff_pool_partials_images(p, 192, 2, 256, 180, None, 1 << 40, None), name)
    _refused(L, L.ff_pool_partials_images(p, 100, 2, 256, 180, p, 1 << 40, None), name)            # ld < C
    _refused(L, L.ff_pool_partials_images(p, 192, 2, 256, 180, p, 2 * 180 - 1, None), name)        # partial buffer: B rows of C
