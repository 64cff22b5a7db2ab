"""Self-ensemble of the tiled C executor, the parts that need no GPU: the four entry points are declared and exported under ABI 7, the
handle-taking ones stay out of the plan dispatcher, and every one refuses bad arguments before any GPU call.  (The tile that
ff_tile_cut_u8_d4 ACCEPTS launches, so that half of the 37x29 / code 4 pair lives in tests/test_image_ens_gpu.py.)"""
import ctypes

import pytest

NEW = ("ff_tile_cut_u8_d4", "ff_tile_fold_d4", "ff_image_ens_workspace_bytes", "ff_forward_image_ens_u8")


@pytest.fixture(scope="module")
def L():
    from isr2_amd.build import build
    from isr2_amd import lib
    build()
    return lib.load()


def test_new_entry_points_are_declared_and_exported(L):
    from isr2_amd import lib
    from isr2_amd.build import LIB
    protos = lib.parse_header()
    raw = ctypes.CDLL(LIB)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/ff_kernels.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
    assert protos["ff_tile_cut_u8_d4"] == ("int", ["const unsigned char*", "int", "int", "int", "int", "int", "int", "int", "float*", "void*"])
    assert protos["ff_tile_fold_d4"] == ("int", ["const float*", "const float*", "int", "int", "int", "float*", "int", "float", "void*"])
    assert protos["ff_image_ens_workspace_bytes"] == ("long long", ["void*", "int", "int"])
    assert protos["ff_forward_image_ens_u8"] == ("int", ["void*", "const unsigned char*", "int", "int", "int", "const int*", "int",
                                                         "unsigned char*", "void*", "long long", "void*"])
    assert L.ff_abi_version() == 7                                  # additive: plans recorded before still load


def test_handle_taking_entries_stay_out_of_the_dispatch_table(tmp_path):
    """A plan may name the two kernels, never the executor's own entries."""
    from isr2_amd.build import gen_dispatch
    p = tmp_path / "ff_dispatch_gen.h"
    gen_dispatch(str(p))
    names = p.read_text().split("FF_DISPATCH_NAMES[FF_DISPATCH_COUNT] = {")[1].split("}")[0]
    assert '"ff_forward_image_ens_u8"' not in names and '"ff_image_ens_workspace_bytes"' not in names
    assert '"ff_forward_image_u8"' not in names and '"ff_image_workspace_bytes"' not in names
    assert '"ff_tile_cut_u8_d4"' in names and '"ff_tile_fold_d4"' in names


def test_executor_entries_refuse_null_arguments(L):
    p = ctypes.c_void_p(4096)                                       # never dereferenced: every call below is refused first
    codes = (ctypes.c_int * 8)(*range(8))
    assert L.ff_image_ens_workspace_bytes(None, 64, 64) == -1 and b"ff_image_ens_workspace_bytes" in L.ff_last_error()
    assert L.ff_forward_image_ens_u8(None, p, 64, 64, 8, codes, 8, p, p, 1 << 30, None) != 0
    assert b"ff_forward_image_ens_u8" in L.ff_last_error()
    assert L.ff_forward_image_ens_u8(p, p, 64, 64, 8, None, 8, p, p, 1 << 30, None) != 0
    assert b"ff_forward_image_ens_u8" in L.ff_last_error()


def test_tile_cut_d4_validates_before_any_launch(L):
    p = ctypes.c_void_p(4096)
    assert L.ff_tile_cut_u8_d4(None, 37, 29, 0, 0, 0, 16, 16, p, None) != 0 and b"ff_tile_cut_u8_d4" in L.ff_last_error()
    assert L.ff_tile_cut_u8_d4(p, 37, 29, 0, 0, 0, 16, 16, None, None) != 0 and b"ff_tile_cut_u8_d4" in L.ff_last_error()
    for code in (16, -1):
        assert L.ff_tile_cut_u8_d4(p, 37, 29, code, 0, 0, 16, 16, p, None) != 0
        assert b"ff_tile_cut_u8_d4" in L.ff_last_error() and str(code).encode() in L.ff_last_error()
    # code 4 turns the 37x29 image into 29x37: row 14 + 16 leaves it (row 13 is the last that fits, see the GPU file)
    assert L.ff_tile_cut_u8_d4(p, 37, 29, 4, 14, 21, 16, 16, p, None) != 0
    err = L.ff_last_error()
    assert b"ff_tile_cut_u8_d4" in err and b"(14,21)" in err and b"29x37" in err and b"37x29" in err, err
    # the same tile fits the untransformed image, so it is the transformed shape that refused it; and the other axis
    assert L.ff_tile_cut_u8_d4(p, 37, 29, 4, 13, 22, 16, 16, p, None) != 0 and b"29x37" in L.ff_last_error()
    assert L.ff_tile_cut_u8_d4(p, 37, 29, 0, 13, 21, 16, 16, p, None) != 0 and b"37x29 transformed" in L.ff_last_error()   # x: 21 + 16 > 29
    for y, x, th, tw in ((-1, 0, 16, 16), (0, -1, 16, 16), (0, 0, 0, 16), (0, 0, 16, 0), (0, 0, 30, 16), (0, 0, 16, 38)):
        assert L.ff_tile_cut_u8_d4(p, 37, 29, 4, y, x, th, tw, p, None) != 0, (y, x, th, tw)
        assert b"ff_tile_cut_u8_d4" in L.ff_last_error()


def test_tile_fold_d4_validates_before_any_launch(L):
    acc, wsum, ens = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20)    # far apart, never dereferenced
    for a, w, e in ((None, wsum, ens), (acc, None, ens), (acc, wsum, None)):
        assert L.ff_tile_fold_d4(a, w, 8, 8, 0, e, 0, 1.0, None) != 0 and b"ff_tile_fold_d4" in L.ff_last_error()
    for code in (16, -1):
        assert L.ff_tile_fold_d4(acc, wsum, 8, 8, code, ens, 0, 1.0, None) != 0
        assert b"ff_tile_fold_d4" in L.ff_last_error() and b"code" in L.ff_last_error()
    assert L.ff_tile_fold_d4(acc, wsum, 8, 8, 0, ens, 2, 1.0, None) != 0 and b"accum" in L.ff_last_error()
    assert L.ff_tile_fold_d4(acc, wsum, 0, 8, 0, ens, 0, 1.0, None) != 0 and b"0x8" in L.ff_last_error()
    assert L.ff_tile_fold_d4(acc, wsum, 8, 8, 0, acc, 0, 1.0, None) != 0 and b"overlaps" in L.ff_last_error()      # ens == acc
    assert L.ff_tile_fold_d4(acc, wsum, 8, 8, 0, wsum, 0, 1.0, None) != 0 and b"overlaps" in L.ff_last_error()     # ens == wsum
    inside = ctypes.c_void_p((1 << 20) + 4 * 8 * 8 * 2)                                                            # ens starts in acc's third plane
    assert L.ff_tile_fold_d4(acc, wsum, 8, 8, 5, inside, 1, 1.0, None) != 0 and b"overlaps" in L.ff_last_error()
