"""Host side of the >= 2^31-element extents of the whole-image path (no GPU).

Coverage closure: every row of tests/golden/bigextent_calls.json -- the launches of one whole-image forward of BASELINE config 4 (a
2040x1356 LR image) with an operand of rows * ld >= 2^30 elements, in bf16x3, bf16 and f32 -- belongs to a launch that is a case of
tests/test_bigextent_gpu.py, to an entry in REFUSED (one that rejects the extent), or to UNPINNED_OPS (named there with a reason; both
lists are empty today).  A new launch in a regenerated table fails this test until it is placed.

Guards: every entry whose kernel keeps 32-bit element offsets refuses an extent at or past 2^31 with FF_ERR_ARG and a message that names
the bound, one element past the largest extent it accepts.  Every call passes host addresses: a call that slipped past a check could not
run a kernel either."""
import ctypes
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
T31 = 2 ** 31


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


def _table():
    with open(os.path.join(HERE, "golden", "bigextent_calls.json")) as f:
        return json.load(f)


def test_table_is_the_config4_forward_in_three_modes():
    t = _table()
    assert t["image"]["lr"] == [1356, 2040] and t["image"]["hr"] == [5424, 8160]
    assert sorted(t["forwards"]) == ["bf16", "bf16x3", "f32"]
    assert all(v["shape"] == [1, 3, 5424, 8160] for v in t["forwards"].values())
    rows = t["rows"]
    assert len(rows) > 100
    for r in rows:
        assert r["extent"] == r["rows"] * r["ld"] and r["ge31"] == (r["extent"] >= T31) and r["ge32"] == (r["extent"] >= 2 ** 32)
        assert r["call"] in t["launches"] and json.loads(r["call"])["op"] == r["op"]
    for call in t["launches"]:                                        # every launch has an operand at or past 2^30: that is why it is here
        assert any(r["call"] == call and r["extent"] >= 2 ** 30 for r in rows), call
    # the pitches the issue names: the hierarchical fusion's in3 (76), EdgeRefine's feats (96), the 64-channel HR tensors
    big = {(r["ld"], r["rows"]) for r in rows if r["ge31"]}
    assert (76, 5424 * 8160) in big and (96, 5424 * 8160) in big and (64, 5424 * 8160) in big


def test_every_row_is_a_gpu_case_a_refusal_or_named_unpinned():
    import test_bigextent_gpu as G
    t = _table()
    placed = {}
    for call in t["launches"]:
        d = json.loads(call)
        where = [n for n, hit in (("case", G.builder_of(d) is not None), ("refused", G.refused(d)), ("unpinned", G.unpinned(d) is not None)) if hit]
        assert len(where) == 1, (where, call)
        placed[call] = where[0]
    for r in t["rows"]:
        assert r["call"] in placed
    cases = {json.dumps(c.launch, sort_keys=True) for c in G.CASES}
    assert cases == {c for c, w in placed.items() if w == "case"}      # the GPU module's case list IS the table's launches
    # nothing past 2^31 is left unpinned without a reason, and the reasons are the documented ones
    for call, w in placed.items():
        if w == "unpinned":
            assert G.unpinned(json.loads(call)) in G.UNPINNED_REASONS


def test_every_case_has_a_geometry_inside_the_recorded_extents():
    """The shape of every GPU case, planned here without a GPU: two whole periods of every marked operand lie past the boundary T, no operand
    outgrows the one the forward produced, and T is not a whole number of periods (a wrapped offset must not land on the same values)."""
    import torch
    import test_bigextent_gpu as G
    from isr2_amd import ops
    prev = ops.gemm_mode()
    try:
        for c in G.CASES:
            ops.set_gemm_mode(c.launch["mode"])
            fam = G.FAMILIES[c.launch["op"]](c.launch, torch.device("cpu"))
            k = G.plan(fam, c.launch, c.T)
            assert k >= 4 and fam.P in (32, 16, 48, 24), c.id
    finally:
        ops.set_gemm_mode(prev)


def test_refused_entries_reject_the_recorded_extent(L, ptr):
    """REFUSED is empty: the config-4 forward itself ran every launch of the table, so no entry in it rejects its extent; the entries that do
    reject such extents never see them (the Python routes fall back or chunk first) and are checked one by one below."""
    import test_bigextent_gpu as G
    assert G.REFUSED == []


# ---- the guards that exist: one call each, every argument valid but the extent -----------------------------------------------------------
def test_conv3x3_halo_refuses_a_2p31_input(L, ptr):
    H, W, ld = 4113, 8160, 64                                           # HR row 4112 (counted from 0) holds element offset 2^31 of a 64-pitch tensor
    assert (H - 1) * W * ld < T31 <= H * W * ld
    w_bytes = L.ff_conv3x3_halo_weight_bytes(64, 64, 64, 3)
    assert w_bytes > 0

    def call(h):
        return L.ff_conv3x3_halo(ptr, ld, ptr, 64, None, None, None, 0, ptr + 64, ld, 1, h, W, 64, 64, 0, 1.0, 0, None, 3, 0, None)
    assert call(H) == 1
    err = L.ff_last_error()
    assert b"ff_conv3x3_halo" in err and b"32-bit offsets" in err, err
    # ops.conv2d never sends such an input: its halo_ok term is the same product
    from isr2_amd import ops
    import inspect
    assert "B * H * W * ldi < 2 ** 31" in inspect.getsource(ops.conv2d)


def test_cab_fused_refuses_2p31_rows(L, ptr):
    import test_cab_fused_entry_cpu as C
    H, W = 3344, 3360                                                   # multiples of 16 at pitch 192: 3344 x 3344 is the last square below 2^31
    assert H * H * 192 < T31 <= H * W * 192
    assert C._call(L, ptr, B=1, H=H, W=W) == 1
    err = L.ff_last_error()
    assert b"ff_cab_fused" in err and b"2^31" in err, err


def test_hab_link_refuses_2p31_rows(L, ptr):
    import test_hab_link_entry_cpu as Hl
    assert 2730 * 4096 * 192 < T31 <= 2731 * 4096 * 192
    assert Hl._call(L, ptr, B=2731, H=64, W=64) == 1
    err = L.ff_last_error()
    assert b"ff_hab_link" in err and b"2^31" in err, err


def test_ocab_attn_refuses_2p31_rows(L, ptr):
    H, W, ldq, ldo = 1984, 2000, 544, 192                               # 1984 * 2000 * 544 = 2.158e9
    assert (H - 16) * W * ldq < T31 <= H * W * ldq
    assert L.ff_ocab_attn(ptr, ldq, 0, 180, 360, ptr + 64, ldo, 0, ptr, 1, H, W, 6, 30, 16, 24, 0.18, 0, None) == 1
    err = L.ff_last_error()
    assert b"ff_ocab_attn" in err and b"32-bit token offsets" in err, err
    ldq16 = 576
    H2 = 1872                                                           # 1872 * 2000 * 576 = 2.157e9 (bf16 elements)
    assert (H2 - 16) * W * ldq16 < T31 <= H2 * W * ldq16
    assert L.ff_ocab_attn_rows16(ptr, ldq16, 0, 192, 384, ptr + 64, ldo, 0, ptr, 1, H2, W, 6, 30, 16, 24, 0, None) == 1
    err = L.ff_last_error()
    assert b"ff_ocab_attn_rows16" in err and b"32-bit token offsets" in err, err


def test_token_projmlp_refuses_2p31_rows(L, ptr):
    M, ld = 11184811, 192                                               # ceil(2^31 / 192)
    assert (M - 1) * ld < T31 <= M * ld
    assert L.ff_token_projmlp(ptr, ld, ptr, ld, None, 0, None, ptr + 64, ld, M, 180, 12, ptr, ptr, ptr, ptr, 1e-5, ptr, ptr, ptr, 3, 0, None) == 1
    err = L.ff_last_error()
    assert b"ff_token_projmlp" in err and b"32-bit row offsets" in err, err


def test_sgfn_tail_refuses_2p31_rows(L, ptr):
    H, W, ldh, c2 = 1425, 2048, 736, 360                                # DAT's fc1 rows at the LR token grid's width (config 4 has 1360 such rows)
    assert (H - 1) * W * ldh < T31 <= H * W * ldh
    assert L.ff_sgfn_tail(ptr, ldh, c2, ptr, ptr, ptr, ptr, None, ptr, 12, None, None, 0, ptr + 64, 192, 1, H, W, 180, None) == 1
    err = L.ff_last_error()
    assert b"ff_sgfn_tail" in err and b"32-bit token offsets" in err, err


def test_row_counts_past_2p31_are_refused_by_the_64_bit_kernels(L, ptr):
    """The implicit GEMMs and ff_layernorm address with 64-bit products of an int row index: what they refuse is a row COUNT past 2^31
    (never reached at config 4: 4.4e7 rows), not an extent."""
    rows = T31
    assert L.ff_layernorm(ptr, 64, ptr + 64, 64, rows, 64, ptr, ptr, 1e-6, None) == 1
    assert b"too many rows" in L.ff_last_error()
    assert L.ff_conv2d(ptr, ptr, None, None, None, ptr + 64, 1, 1 << 16, 1 << 15, 64, 64, 1 << 16, 1 << 15, 64, 64, 0, 1, 1, 1, 1, 0, 0, 0, 1.0, 0, 0, None) == 1
    assert b"M overflows int" in L.ff_last_error()
