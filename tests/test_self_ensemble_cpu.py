"""Host side of the x8 geometric self-ensemble: the code algebra of the eight symmetries (ops.d4_inverse_code, ops.D4_ENSEMBLE) against
torch's flip / rot90, and the argument checks of ff_d4_rect_nchw, which return before any launch (this runs without a GPU)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_d4(x, code):
    """The transform a d4 code names, restated with torch: flip(-1), then flip(-2), then rot90(k)."""
    if code & 1:
        x = x.flip(-1)
    if code & 2:
        x = x.flip(-2)
    return torch.rot90(x, code >> 2, dims=(-2, -1))


@pytest.fixture(scope="module")
def probe():
    return torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7)


def test_inverse_code_undoes_every_code(probe):
    from isr2_amd import ops
    for c in range(16):
        ic = ops.d4_inverse_code(c)
        assert isinstance(ic, int) and 0 <= ic < 16
        back = torch_d4(torch_d4(probe, c), ic)
        assert back.shape == probe.shape and torch.equal(back, probe), (c, ic)
    for bad in (-1, 16):
        with pytest.raises(ops._lib.FFError):
            ops.d4_inverse_code(bad)


def test_ensemble_codes_are_the_eight_distinct_symmetries(probe):
    from isr2_amd import ops
    assert tuple(ops.D4_ENSEMBLE) == (0, 1, 2, 3, 4, 5, 6, 7)
    imgs = [torch_d4(probe, c) for c in ops.D4_ENSEMBLE]
    for i in range(8):
        for j in range(i):
            assert imgs[i].shape != imgs[j].shape or not torch.equal(imgs[i], imgs[j]), (i, j)
    for c in range(16):                                           # codes 8..15 repeat them, and the canonical code says which
        cc = ops.d4_canonical_code(c)
        assert cc in ops.D4_ENSEMBLE and torch.equal(torch_d4(probe, c), torch_d4(probe, cc)), (c, cc)


def test_d4_rect_argument_validation_needs_no_gpu():
    from isr2_amd import lib as L
    lib = L.load()
    a = (ctypes.c_float * 64)()
    b = (ctypes.c_float * 64)()
    pa, pb = ctypes.addressof(a), ctypes.addressof(b)             # host memory: every call below must return before any launch
    cases = {
        "null src": (None, pb, 1, 1, 4, 4, 0, 0, 1.0, None),
        "null dst": (pa, None, 1, 1, 4, 4, 0, 0, 1.0, None),
        "src == dst": (pa, pa, 1, 1, 4, 4, 0, 0, 1.0, None),
        "code 16": (pa, pb, 1, 1, 4, 4, 16, 0, 1.0, None),
        "code -1": (pa, pb, 1, 1, 4, 4, -1, 0, 1.0, None),
        "Hs = 0": (pa, pb, 1, 1, 0, 4, 0, 0, 1.0, None),
        "Ws = 0": (pa, pb, 1, 1, 4, 0, 4, 0, 1.0, None),
        "accum 2": (pa, pb, 1, 1, 4, 4, 0, 2, 1.0, None),
        "grid": (pa, pb, 1 << 15, 1 << 15, 65, 65, 4, 0, 1.0, None),   # 2^30 planes x 4 tiles = 2^32 blocks
    }
    for what, args in cases.items():
        rc = lib.ff_d4_rect_nchw(*args)
        assert rc != 0 and b"ff_d4_rect_nchw" in lib.ff_last_error(), what


def test_header_declares_d4_rect_and_abi_stays_7():
    from isr2_amd import lib as L
    protos = L.parse_header()
    assert protos["ff_d4_rect_nchw"] == ("int", ["const float*", "float*", "int", "int", "int", "int", "int", "int", "float", "void*"])
    assert protos["ff_d4_nchw"] == ("int", ["const float*", "float*", "int", "int", "int", "int", "const int*", "void*"])   # untouched
    assert L.load().ff_abi_version() == 7
    hdr = open(os.path.join(ROOT, "include", "ff_kernels.h")).read()
    assert re.search(r"int\s+ff_d4_rect_nchw\s*\(", hdr)


def test_plugin_switch_parsing(monkeypatch):
    import models.team29_FreqFusion.io as plug
    for v, want in ((None, False), ("", False), ("0", False), ("1", True), ("8", True)):
        if v is None:
            monkeypatch.delenv("FF_SELF_ENSEMBLE", raising=False)
        else:
            monkeypatch.setenv("FF_SELF_ENSEMBLE", v)
        assert plug._self_ensemble_on() is want, v
    monkeypatch.setenv("FF_SELF_ENSEMBLE", "4")
    with pytest.raises(ValueError):
        plug._self_ensemble_on()
