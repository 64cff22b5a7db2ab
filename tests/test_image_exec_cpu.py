"""Tiled C executor, the parts that need no GPU: the six entry points are declared and exported, ff_tile_positions reproduces the
plugin's _tile_positions, and every entry point refuses bad arguments before any GPU call."""
import ctypes

import pytest

NEW = ("ff_tile_positions", "ff_tile_cut_u8", "ff_tile_ramps", "ff_tile_finish_u8", "ff_image_workspace_bytes", "ff_forward_image_u8")


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
    assert protos["ff_tile_positions"] == ("int", ["int", "int", "int", "int*", "int"])
    assert protos["ff_image_workspace_bytes"][0] == "long long"
    assert L.ff_abi_version() == 7                                  # additive: plans recorded before still load


def test_handle_taking_entry_stays_out_of_the_dispatch_table(tmp_path):
    """A plan names entry points of the generated dispatch table only; the executor's own entries must never be among them."""
    from isr2_amd.build import gen_dispatch
    p = tmp_path / "ff_dispatch_gen.h"
    gen_dispatch(str(p))
    names = p.read_text().split("FF_DISPATCH_NAMES[FF_DISPATCH_COUNT] = {")[1].split("}")[0]
    assert '"ff_forward_image_u8"' not in names and '"ff_forward"' not in names and '"ff_image_workspace_bytes"' not in names
    assert '"ff_tile_cut_u8"' in names and '"ff_tile_finish_u8"' in names


def _positions(L, n, tile, step, cap=4096):
    buf = (ctypes.c_int * max(cap, 1))()
    cnt = L.ff_tile_positions(n, tile, step, buf, cap)
    return cnt, list(buf[:max(cnt, 0)])


def test_tile_positions_equal_the_plugins(L):
    import models.team29_FreqFusion.io as plug
    seen = 0
    for tile in (16, 128):
        for n in (tile, tile + 1, 2 * tile - 1, 37, 29, 510, 339):
            for step in range(1, tile + 1):
                cnt, got = _positions(L, n, tile, step)
                if n < tile:
                    assert cnt == -1, (n, tile, step)
                    continue
                want = plug._tile_positions(n, tile, step)
                assert cnt == len(want) and got == want, (n, tile, step, got, want)
                assert got[0] == 0 and got[-1] + tile == n          # the last tile sits flush to the border
                seen += 1
    assert seen == 7 * 16 + 5 * 128                                # 37 and 29 are smaller than the 128 tile


def test_tile_positions_refusals(L):
    assert _positions(L, 15, 16, 4)[0] == -1                       # n < tile
    assert _positions(L, 37, 16, 0)[0] == -1                       # step = 0
    assert _positions(L, 37, 0, 4)[0] == -1                        # tile < 1
    want = [0, 12, 21]
    assert _positions(L, 37, 16, 12) == (3, want)
    assert _positions(L, 37, 16, 12, cap=3) == (3, want)
    assert _positions(L, 37, 16, 12, cap=2)[0] == -1               # the flush-to-border tile does not fit
    assert _positions(L, 37, 16, 12, cap=1)[0] == -1
    assert L.ff_tile_positions(37, 16, 12, None, 8) == -1


def test_kernel_entries_validate_before_any_launch(L):
    p = ctypes.c_void_p(4096)                                       # never dereferenced: every call below is refused first
    assert L.ff_tile_cut_u8(None, 37, 29, 0, 0, 16, 16, p, None) != 0 and b"ff_tile_cut_u8" in L.ff_last_error()
    assert L.ff_tile_cut_u8(p, 37, 29, 0, 0, 16, 16, None, None) != 0 and b"ff_tile_cut_u8" in L.ff_last_error()
    for y, x, th, tw in ((22, 0, 16, 16), (0, 14, 16, 16), (-1, 0, 16, 16), (0, -1, 16, 16), (0, 0, 38, 16), (0, 0, 16, 30), (0, 0, 0, 16)):
        assert L.ff_tile_cut_u8(p, 37, 29, y, x, th, tw, p, None) != 0, (y, x, th, tw)
        assert b"ff_tile_cut_u8" in L.ff_last_error()
    assert L.ff_tile_cut_u8(p, 37, 29, 22, 0, 16, 16, p, None) != 0 and b"leaves the 37x29 image" in L.ff_last_error()

    assert L.ff_tile_ramps(None, 64, 16, None) != 0 and b"ff_tile_ramps" in L.ff_last_error()
    assert L.ff_tile_ramps(p, 64, 65, None) != 0 and b"ff_tile_ramps" in L.ff_last_error() and b"65" in L.ff_last_error()
    assert L.ff_tile_ramps(p, 64, -1, None) != 0 and b"ff_tile_ramps" in L.ff_last_error()

    assert L.ff_tile_finish_u8(None, p, 4, 4, p, None) != 0 and b"ff_tile_finish_u8" in L.ff_last_error()
    assert L.ff_tile_finish_u8(p, None, 4, 4, p, None) != 0 and b"ff_tile_finish_u8" in L.ff_last_error()
    assert L.ff_tile_finish_u8(p, p, 4, 4, None, None) != 0 and b"ff_tile_finish_u8" in L.ff_last_error()
    assert L.ff_tile_finish_u8(p, p, 0, 4, p, None) != 0 and b"ff_tile_finish_u8" in L.ff_last_error()


def test_executor_entries_refuse_a_null_handle(L):
    p = ctypes.c_void_p(4096)
    assert L.ff_image_workspace_bytes(None, 64, 64) == -1 and b"ff_image_workspace_bytes" in L.ff_last_error()
    assert L.ff_forward_image_u8(None, p, 64, 64, 8, p, p, 1 << 30, None) != 0
    assert b"ff_forward_image_u8" in L.ff_last_error()
