"""Host side of the fusion stack's per-image entry points (no GPU): the new symbols, the FFT workspace helper, and the checks that
refuse a launch.  The geometry check is every entry point's FIRST check and uses host values only, so the calls below -- host
addresses, null pointers -- cannot reach a launch; the later checks (null pointers, workspace, ldo) are host-only too."""
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


def _refused(L, status, name, word=None):
    assert status == 1, name                                     # FF_ERR_ARG
    err = L.ff_last_error()
    assert name.encode() + b":" in err, err
    if word is not None:
        assert word.encode() in err, err


NEW = ("ff_dct8_bands_images", "ff_fft_bands_images", "ff_fft_bands_images_workspace", "ff_fuse_blend_images", "ff_mix2_images")


def test_new_symbols_are_declared_and_exported(L):
    from isr2_amd.lib import parse_header
    protos = parse_header()
    for name in NEW:
        assert name in protos, name
        assert getattr(L, name) is not None
    assert L.ff_abi_version() == 7                               # additive entry points: the version stays
    from isr2_amd import ops
    import inspect
    assert "rows_per_image" in inspect.signature(ops.linear).parameters


@pytest.mark.parametrize("H,W", [(2, 2), (8, 8), (17, 19), (20, 40), (64, 64), (256, 256), (481, 8192), (600, 333), (1638, 9)])
def test_fft_workspace_is_b_times_one_image(L, H, W):
    one = 4 * 3 * H * (W // 2 + 1)                               # what ops.fft_bands allocates for ff_fft_bands with C = 3
    assert L.ff_fft_bands_images_workspace(1, H, W) == one
    for B in (2, 5, 16, 21845):
        assert L.ff_fft_bands_images_workspace(B, H, W) == B * one
    for B in (0, -3, 21846, 70000):                              # 3 B > 65535: the planes index gridDim.y
        assert L.ff_fft_bands_images_workspace(B, H, W) == -1


def test_fft_workspace_refuses_sizes_below_the_single_image_minimum(L):
    for H, W in ((1, 8), (8, 1), (0, 8), (8, 0), (-4, 8), (8, 8193), (482, 8), (512, 8), (1639, 8), (8193, 8)):        # (H: the column tile of ff_fft_bands must fit 64 KiB of LDS)
        assert L.ff_fft_bands_images_workspace(2, H, W) == -1, (H, W)


# B, H, W the DCT form refuses first
BAD_DCT = [(0, 8, 8), (-1, 8, 8), (21846, 8, 8), (70000, 8, 8), (2, 7, 8), (2, 8, 7), (2, 0, 16), (2, 16, -8)]
BAD_FFT = [(0, 8, 8), (-1, 8, 8), (21846, 8, 8), (70000, 8, 8), (2, 1, 8), (2, 8, 1), (2, 0, 16), (2, 16, -8), (2, 500, 16), (2, 1639, 16), (2, 16, 8193)]


def test_dct8_bands_images_refusals(L, p):
    name = "ff_dct8_bands_images"

    def call(x=p, D=p, m=p, s=p, out=p, B=2, H=8, W=8, ldo=27, off=0):
        return L.ff_dct8_bands_images(x, B, H, W, D, m, s, out, ldo, off, None)

    for B, H, W in BAD_DCT:
        _refused(L, call(B=B, H=H, W=W), name, "expects")
        _refused(L, call(B=B, H=H, W=W, x=None, D=None, out=None, ldo=0), name, "expects")       # null pointers behind the check
    for kw in (dict(x=None), dict(D=None), dict(m=None), dict(s=None), dict(out=None)):
        _refused(L, call(**kw), name, "null pointer")
    _refused(L, call(ldo=8), name, "ldo")                        # nine channels are written
    _refused(L, call(ldo=27, off=19), name, "ldo")
    _refused(L, call(off=-1), name, "ldo")


def test_fft_bands_images_refusals(L, p):
    name = "ff_fft_bands_images"
    need = L.ff_fft_bands_images_workspace(2, 8, 8)
    assert need == 2 * 4 * 3 * 8 * 5

    def call(x=p, tw=p, mask=p, sc=p, work=p, out=p, B=2, H=8, W=8, nwork=None, ldo=27, lo=21, hi=24):
        return L.ff_fft_bands_images(x, B, H, W, tw, tw, tw, tw, mask, 64, 1.0, sc, work, need if nwork is None else nwork, out, ldo, lo, hi, None)

    for B, H, W in BAD_FFT:
        _refused(L, call(B=B, H=H, W=W, nwork=1 << 40), name, "expects")
        _refused(L, call(B=B, H=H, W=W, nwork=0, x=None, work=None, out=None, ldo=0), name, "expects")
    for kw in (dict(x=None), dict(tw=None), dict(mask=None), dict(sc=None), dict(work=None), dict(out=None)):
        _refused(L, call(**kw), name, "null pointer")
    _refused(L, call(nwork=need - 1), name, "workspace")         # one float short
    _refused(L, call(ldo=26), name, "ldo")                       # channels 24..26 are written
    _refused(L, call(ldo=5, lo=0, hi=3), name, "ldo")
    _refused(L, call(lo=-1), name, "ldo")


def test_fuse_blend_images_refusals(L, p):
    name = "ff_fuse_blend_images"

    def call(e=p, h=p, g=p, t=p, d=p, o=p, B=2, Hh=32, Wh=32, Hl=8, Wl=8):
        return L.ff_fuse_blend_images(e, h, g, t, d, o, B, Hh, Wh, Hl, Wl, None)

    for kw in (dict(B=0), dict(B=-2), dict(B=65536), dict(Hh=0), dict(Wh=-1), dict(Hl=0), dict(Wl=0)):
        _refused(L, call(**kw), name, "expects")
        _refused(L, call(e=None, h=None, o=None, **kw), name, "expects")
    for kw in (dict(e=None), dict(h=None), dict(g=None), dict(t=None), dict(d=None), dict(o=None)):
        _refused(L, call(**kw), name, "null pointer")


def test_mix2_images_refusals(L, p):
    name = "ff_mix2_images"

    def call(out=p, a=p, ca=p, rows=512, C=3, B=2, rpi=256, ldo=9, lda=9):
        return L.ff_mix2_images(out, ldo, a, lda, None, 0, rows, C, 1.0, 1.0, ca, B, rpi, None, None, 0, None, 0, 1, None)

    for kw in (dict(B=0), dict(B=-1), dict(rpi=0), dict(rows=511), dict(rows=768), dict(B=3)):
        _refused(L, call(**kw), name, "rows_per_image")
        _refused(L, call(out=None, a=None, ca=None, **kw), name, "rows_per_image")
    for kw in (dict(out=None), dict(a=None), dict(ca=None), dict(C=0), dict(ldo=2), dict(lda=2)):
        _refused(L, call(**kw), name, "bad args")
