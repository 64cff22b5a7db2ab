"""x8 self-ensemble of the tiled C executor on the GPU: ff_tile_cut_u8_d4 and ff_tile_fold_d4 against the launches they replace, and
ff_forward_image_ens_u8 (a [2,3,16,16] tile plan, uint8 in and out) against model.self_ensemble run over the plugin's own
_tiled_forward.  torch.equal throughout."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CODES8 = (0, 1, 2, 3, 4, 5, 6, 7)


def _a256(n):
    return (n + 255) // 256 * 256


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import lib
    return lib.load()


def _image(seed, H, W):
    """The generator of tests/test_image_exec_gpu.py: 0 and 255 are both present."""
    img = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[0, 0, 0], img[-1, -1, 2], img[H // 2, W // 2, 1] = 0, 255, 255
    return torch.from_numpy(img).cuda()


# ---- ff_tile_cut_u8_d4 ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def img37(L):
    from isr2_amd import ops
    img = _image(11, 37, 29)
    assert int(img.min()) == 0 and int(img.max()) == 255
    return img, ops.u8_to_f32_image(img)


@pytest.mark.parametrize("code", CODES8 + (13,))
def test_tile_cut_d4_equals_convert_transform_slice(L, img37, code):
    """37x29 image: every code against d4_rect of the converted image, sliced.  16x16 tiles at the origin, at the far corner of the
    TRANSFORMED shape and at four columns that bring every byte alignment of a row start; a tall 32x8 tile where the shape holds it."""
    from isr2_amd import ops
    img, full = img37
    H, W, _ = img.shape
    want = ops.d4_rect(full, code)
    Ht, Wt = want.shape[-2:]
    assert (Ht, Wt) == ((W, H) if (code >> 2) & 1 else (H, W))
    tiles = [(0, 0, 16, 16), (Ht - 16, Wt - 16, 16, 16), (5, 1, 16, 16), (5, 2, 16, 16), (5, 3, 16, 16), (5, 4, 16, 16)]
    if Ht >= 32:
        tiles.append((Ht - 32, Wt - 8, 32, 8))
    for y, x, th, tw in tiles:
        out = torch.full((1, 3, th, tw), -1.0, device="cuda")
        assert L.ff_tile_cut_u8_d4(img.data_ptr(), H, W, code, y, x, th, tw, out.data_ptr(), _stream()) == 0, L.ff_last_error()
        assert torch.equal(out, want[..., y:y + th, x:x + tw]), (code, y, x, th, tw)
        assert torch.equal(ops.tile_cut_u8_d4(img, code, y, x, th, tw), out)
    # one row / one column past the far corner: refused, out untouched
    keep = torch.full((1, 3, 16, 16), -1.0, device="cuda")
    out = keep.clone()
    for y, x in ((Ht - 15, Wt - 16), (Ht - 16, Wt - 15)):
        assert L.ff_tile_cut_u8_d4(img.data_ptr(), H, W, code, y, x, 16, 16, out.data_ptr(), _stream()) != 0
        assert f"leaves the {Ht}x{Wt} transformed image".encode() in L.ff_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, keep), "a refused cut wrote to out"


def test_tile_cut_d4_code4_tile_flush_to_the_transformed_border(L, img37):
    """The accepted half of the CPU file's pair: code 4 turns 37x29 into 29x37, (13, 21) is its last 16x16 tile; (14, 21) leaves it."""
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    img, full = img37
    out = torch.full((1, 3, 16, 16), -1.0, device="cuda")
    assert L.ff_tile_cut_u8_d4(img.data_ptr(), 37, 29, 4, 13, 21, 16, 16, out.data_ptr(), _stream()) == 0, L.ff_last_error()
    assert torch.equal(out, ops.d4_rect(full, 4)[..., 13:29, 21:37])
    with pytest.raises(FFError, match="29x37"):
        ops.tile_cut_u8_d4(img, 4, 14, 21, 16, 16)
    with pytest.raises(FFError, match="d4 code 16"):
        ops.tile_cut_u8_d4(img, 16, 0, 0, 16, 16)


# ---- ff_tile_fold_d4 -----------------------------------------------------------------------------------------------------------
def _d4_tile():
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "image-super-resolution-2_amd", "csrc", "d4_tile.inc")
    return int(re.search(r"#define D4_TILE (\d+)", open(src).read()).group(1))


def _canvases():
    T = _d4_tile()
    edge = (33, 65) if T <= 32 else (T + 1, 2 * T + 1)          # straddles the LDS tile edge on both axes
    return [(1, 1), (3, 5), edge, (64, 68)]


@pytest.mark.parametrize("Hc,Wc", _canvases())
def test_tile_fold_equals_normalize_then_d4_rect(L, Hc, Wc):
    """Every code 0..7 and 13, accum 0 and 1 (on a pre-filled ens), scale 1, 1/8 and float(1/3), against ops.tile_normalize on a clone
    followed by ops.d4_rect.  wsum holds 0 (the 1e-8 clamp, under a non-trivial acc), 0.25, 1 and 2; acc and wsum stay as they
    were and the floats around ens are not written."""
    from isr2_amd import ops
    rng = np.random.default_rng(1000 * Hc + Wc)
    wsum = torch.from_numpy(rng.choice(np.array([0.0, 0.25, 1.0, 2.0], dtype=np.float32), size=(1, 1, Hc, Wc))).cuda()
    if Hc * Wc >= 4:
        wsum.view(-1)[:4] = torch.tensor([0.0, 0.25, 1.0, 2.0], device="cuda")
        assert set(wsum.unique().tolist()) == {0.0, 0.25, 1.0, 2.0}
    else:
        wsum.zero_()
    acc = torch.from_numpy(rng.uniform(-0.2, 1.3, (1, 3, Hc, Wc)).astype(np.float32)).cuda()
    assert bool((acc[:, :, wsum[0, 0] == 0] != 0).all())
    acc0, wsum0 = acc.clone(), wsum.clone()
    norm = acc.clone()
    ops.tile_normalize(norm, wsum)
    prefill = torch.from_numpy(rng.uniform(-1.0, 2.0, (3 * Hc * Wc,)).astype(np.float32)).cuda()
    G = 64                                                         # guard floats on either side of ens
    buf = torch.empty(3 * Hc * Wc + 2 * G, device="cuda")
    guard = float(np.float32(-12345.5))
    for code in CODES8 + (13,):
        oshape = (1, 3, Wc, Hc) if (code >> 2) & 1 else (1, 3, Hc, Wc)
        for accum in (0, 1):
            for scale in (1.0, 0.125, float(1 / 3)):
                buf.fill_(guard)
                ens = buf[G:G + 3 * Hc * Wc].view(oshape)
                ens.view(-1).copy_(prefill)
                ref = prefill.clone().view(oshape)
                ops.d4_rect(norm, code, out=ref, accum=bool(accum), scale=scale)
                rc = L.ff_tile_fold_d4(acc.data_ptr(), wsum.data_ptr(), Hc, Wc, code, ens.data_ptr(), accum, scale, _stream())
                assert rc == 0, L.ff_last_error()
                assert torch.equal(ens, ref), (code, accum, scale, int((ens != ref).sum()))
                assert bool((buf[:G] == guard).all()) and bool((buf[G + 3 * Hc * Wc:] == guard).all()), "floats outside ens were written"
    assert torch.equal(acc, acc0) and torch.equal(wsum, wsum0), "ff_tile_fold_d4 must leave acc and wsum untouched"
    # the wrapper: allocates ens, refuses an overlapping or mis-shaped one
    from isr2_amd.lib import FFError
    assert torch.equal(ops.tile_fold_d4(acc, wsum, 5, scale=0.125), ops.d4_rect(norm, 5, scale=0.125))
    with pytest.raises(FFError, match="overlaps acc"):
        ops.tile_fold_d4(acc, wsum, 0, ens=acc)
    with pytest.raises(FFError, match="accum=True"):
        ops.tile_fold_d4(acc, wsum, 0, accum=True)


def test_tile_fold_unaligned_planes_take_the_scalar_path(L):
    """64x68 is a multiple of 4 wide, but an ens that starts 4 bytes past a 16-byte boundary must not be stored as float4."""
    from isr2_amd import ops
    Hc, Wc = 64, 68
    rng = np.random.default_rng(7)
    wsum = torch.from_numpy(rng.choice(np.array([0.25, 1.0, 2.0], dtype=np.float32), size=(1, 1, Hc, Wc))).cuda()
    acc = torch.from_numpy(rng.uniform(-0.2, 1.3, (1, 3, Hc, Wc)).astype(np.float32)).cuda()
    norm = acc.clone()
    ops.tile_normalize(norm, wsum)
    buf = torch.zeros(3 * Hc * Wc + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    for code in (0, 3, 5):
        ens = buf[1:1 + 3 * Hc * Wc].view(1, 3, *((Wc, Hc) if code & 4 else (Hc, Wc)))
        assert L.ff_tile_fold_d4(acc.data_ptr(), wsum.data_ptr(), Hc, Wc, code, ens.data_ptr(), 0, 1.0, _stream()) == 0, L.ff_last_error()
        assert torch.equal(ens, ops.d4_rect(norm, code))
        assert float(buf[0]) == 0.0 and bool((buf[1 + 3 * Hc * Wc:] == 0).all())


# ---- end to end ----------------------------------------------------------------------------------------------------------------
TILE, BATCH = 16, 2


def _drop_graphs(model):
    from isr2_amd import ops
    torch.cuda.synchronize()
    for key in list(model._graphs):
        model._graphs.pop(key)
        ops.drop_persistent(key=(id(model),) + key)


class _Ctx:
    pass


@pytest.fixture(scope="module", params=["bf16x3", "bf16"])
def ctx(request, L, synth_sd, tmp_path_factory):
    from isr2_amd import ops, plan
    from isr2_amd.model import FreqFusionHIP
    prev = ops.gemm_mode()
    ops.set_gemm_mode(request.param)
    c = _Ctx()
    c.mode, c.L = request.param, L
    c.model = FreqFusionHIP(synth_sd, "cuda:0")                    # per mode: the model's graph cache is keyed by shape only
    c.dir = tmp_path_factory.mktemp("ensplan_" + request.param)
    c.pair = torch.from_numpy(np.random.default_rng(21).random((BATCH, 3, TILE, TILE), dtype=np.float32)).cuda()
    stem = str(c.dir / "t16b2")
    c.info = plan.export_plan(c.model, c.pair, stem)
    c.nat = plan.NativeModel(stem + ".ffplan", stem + ".ffwts")
    c.img = _image(31, 37, 29)
    c.want = {}                                                    # (overlap, codes) -> the Python ensemble, computed once
    try:
        yield c
    finally:
        c.nat.close()
        _drop_graphs(c.model)
        ops.set_gemm_mode(prev)


def _python_ensemble(ctx, img, overlap, codes):
    """The expression the entry point is pinned to: model.self_ensemble with the plugin's tiled forward as `run`."""
    import models.team29_FreqFusion.io as plug
    from isr2_amd import ops
    key = (tuple(img.shape), overlap, tuple(codes))
    if key not in ctx.want:
        dev = torch.device("cuda:0")
        lr = ops.u8_to_f32_image(img)
        ens = ctx.model.self_ensemble(lr, codes=codes, run=lambda v: plug._tiled_forward(ctx.model, v, TILE, overlap, 4, dev)).clone()
        ctx.want[key] = (ens, ops.f32_to_u8_image(ens))
    return ctx.want[key]


def _plain_bytes(H, W):
    return _a256(12 * 16 * H * W) + _a256(4 * 16 * H * W) + _a256(12 * BATCH * TILE * TILE) + _a256(12 * BATCH * 16 * TILE * TILE) + _a256(16 * 4 * TILE)


def _expected_bytes(H, W):
    """include/ff_kernels.h: the parts of ff_forward_image_u8, then ens [3][4H][4W] fp32, every part padded to 256 bytes."""
    return _plain_bytes(H, W) + _a256(12 * 16 * H * W)


def _ens_view(work, H, W):
    o = _plain_bytes(H, W)
    return work[o:o + 12 * 16 * H * W].view(torch.float32).view(1, 3, 4 * H, 4 * W)


@pytest.mark.parametrize("overlap,codes,ntiles", [(4, CODES8, 9), (6, (0, 6, 3), 12)])
def test_image_ensemble_equals_self_ensemble_over_the_plugins_tiled_forward(ctx, overlap, codes, ntiles):
    """37x29 through [2,3,16,16].  Overlap 4: 3x3 tiles per variant in BOTH orientations (odd: the last group is padded with a
    repeat), all eight symmetries, scale 1/8.  Overlap 6: 4x3 / 3x4 tiles, the capped blend, three codes and float(1/3) as the scale.
    The uint8 image AND the fp32 ens part of work must equal the Python path."""
    import models.team29_FreqFusion.io as plug
    from isr2_amd import ops
    assert ops.gemm_mode() == ctx.mode
    H, W, _ = ctx.img.shape
    step = TILE - overlap
    assert len(plug._tile_positions(H, TILE, step)) * len(plug._tile_positions(W, TILE, step)) == ntiles
    want_f, want = _python_ensemble(ctx, ctx.img, overlap, codes)
    need = ctx.nat.image_ens_workspace_bytes(H, W)
    assert need == _expected_bytes(H, W) and need == ctx.nat.image_workspace_bytes(H, W) + _a256(12 * 16 * H * W)
    work = torch.full((need,), 0xFF, device="cuda", dtype=torch.uint8)      # NaN bit patterns: nothing may be read before it is written
    got = ctx.nat.forward_image_ens_u8(ctx.img, overlap=overlap, codes=codes, work=work)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4 * H, 4 * W, 3)
    assert torch.equal(got, want), f"{int((got != want).sum())} bytes differ"
    assert torch.equal(_ens_view(work, H, W), want_f), "the fp32 ensemble differs from model.self_ensemble"
    # a second call on the dirty buffer, and the default buffer
    assert torch.equal(ctx.nat.forward_image_ens_u8(ctx.img, overlap=overlap, codes=codes, work=work), want)
    assert torch.equal(_ens_view(work, H, W), want_f)
    if codes == CODES8:                                            # codes defaults to ops.D4_ENSEMBLE
        assert tuple(ops.D4_ENSEMBLE) == CODES8
        assert torch.equal(ctx.nat.forward_image_ens_u8(ctx.img, overlap=overlap), want)
    else:
        assert torch.equal(ctx.nat.forward_image_ens_u8(ctx.img, overlap=overlap, codes=codes), want)


def test_ensemble_of_one_tile_equals_the_untiled_self_ensemble(ctx):
    from isr2_amd import ops
    img = _image(32, TILE, TILE)
    lr = ops.u8_to_f32_image(img)
    want = ops.f32_to_u8_image(ctx.model.self_ensemble(lr))
    assert torch.equal(ctx.nat.forward_image_ens_u8(img, overlap=4), want)


def test_single_code_equals_the_plain_image_call(ctx):
    want = ctx.nat.forward_image_u8(ctx.img, overlap=4)
    assert torch.equal(ctx.nat.forward_image_ens_u8(ctx.img, overlap=4, codes=(0,)), want)


def test_codes_1_and_9_are_two_symmetries_here_as_in_self_ensemble(ctx):
    """hflip and hflip + half turn (= vflip, canonical code 2) are different symmetries: the pair is accepted, as model.self_ensemble
    accepts it, and gives its bytes (scale 1/2, one code from 8..15)."""
    want_f, want = _python_ensemble(ctx, ctx.img, 4, (1, 9))
    assert torch.equal(ctx.nat.forward_image_ens_u8(ctx.img, overlap=4, codes=(1, 9)), want)


def test_ensemble_call_is_graph_capturable(ctx):
    H, W, _ = ctx.img.shape
    codes = (ctypes.c_int * 2)(0, 5)
    want = ctx.nat.forward_image_ens_u8(ctx.img, overlap=4, codes=(0, 5))
    work = torch.empty(ctx.nat.image_ens_workspace_bytes(H, W), device="cuda", dtype=torch.uint8)
    static_in = ctx.img.clone()
    static_out = torch.zeros_like(want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = ctx.L.ff_forward_image_ens_u8(ctx.nat.h, static_in.data_ptr(), H, W, 4, codes, 2, static_out.data_ptr(), work.data_ptr(),
                                           work.numel(), _stream())
    assert rc == 0, ctx.L.ff_last_error()
    for _ in range(2):
        static_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, want)
    del g


def test_ensemble_refusals_name_the_sizes_and_write_nothing(ctx, tmp_path):
    from isr2_amd import ops, plan
    from isr2_amd.lib import FFError
    L, nat = ctx.L, ctx.nat
    H, W, _ = ctx.img.shape
    need = nat.image_ens_workspace_bytes(H, W)
    work = torch.empty(need, device="cuda", dtype=torch.uint8)
    out = torch.full((4 * 40, 4 * 40, 3), 0x5A, device="cuda", dtype=torch.uint8)

    def refused(handle, img, h, w, overlap, codes, nbytes, *words):
        arr = (ctypes.c_int * max(len(codes), 1))(*codes)
        rc = L.ff_forward_image_ens_u8(handle, img.data_ptr(), h, w, overlap, arr, len(codes), out.data_ptr(), work.data_ptr(), nbytes, _stream())
        err = L.ff_last_error().decode()
        assert rc != 0 and "ff_forward_image_ens_u8" in err, err
        for wd in words:
            assert wd in err, (wd, err)
        torch.cuda.synchronize()
        assert bool((out == 0x5A).all()), "a refused call wrote to out"

    small = _image(33, 15, 40)
    refused(nat.h, ctx.img, H, W, 4, (), need, "ncodes = 0")
    refused(nat.h, ctx.img, H, W, 4, (0, 16), need, "codes[1] = 16", "0..15")
    # two codes that name one symmetry, compared as ops.d4_canonical_code does: 10 (vflip + half turn) is 1, 9 (hflip + half turn) is 2
    assert ops.d4_canonical_code(10) == 1 and ops.d4_canonical_code(9) == 2
    refused(nat.h, ctx.img, H, W, 4, (1, 10), need, "codes[0] = 1", "codes[1] = 10", "same symmetry")
    refused(nat.h, ctx.img, H, W, 4, (0, 2, 9), need, "codes[1] = 2", "codes[2] = 9", "same symmetry")
    with pytest.raises(FFError, match="twice"):
        ctx.model.self_ensemble(ops.u8_to_f32_image(ctx.img), codes=(1, 10), run=lambda v: v)
    refused(nat.h, small, 15, 40, 4, CODES8, need, "15x40", "16x16", "ragged")
    refused(nat.h, ctx.img, H, W, 16, CODES8, need, "overlap 16", "16")
    refused(nat.h, ctx.img, H, W, 4, CODES8, need - 1, "37x29", str(need), str(need - 1))
    with pytest.raises(FFError, match="ncodes = 0"):
        nat.forward_image_ens_u8(ctx.img, overlap=4, codes=())
    with pytest.raises(FFError, match="same symmetry"):
        nat.forward_image_ens_u8(ctx.img, overlap=4, codes=(1, 10))
    with pytest.raises(FFError, match="15x40"):
        nat.forward_image_ens_u8(small, overlap=4)
    with pytest.raises(FFError, match="15x40"):
        nat.image_ens_workspace_bytes(15, 40)
    with pytest.raises(FFError, match=str(need - 1)):
        nat.forward_image_ens_u8(ctx.img, overlap=4, work=work[:need - 1])
    with pytest.raises(FFError):
        nat.forward_image_ens_u8(ctx.img.float())

    # a plan with a non-square tile is no tile plan
    stem = str(tmp_path / "t16x24")
    lr = torch.from_numpy(np.random.default_rng(22).random((1, 3, 16, 24), dtype=np.float32)).cuda()
    plan.export_plan(ctx.model, lr, stem, verify=False)
    rect = plan.NativeModel(stem + ".ffplan", stem + ".ffwts")
    try:
        refused(rect.h, ctx.img, H, W, 4, CODES8, need, "[1,3,16,24]", "[1,3,64,96]")
        with pytest.raises(FFError, match=r"\[1,3,16,24\]"):
            rect.image_ens_workspace_bytes(H, W)
    finally:
        rect.close()
    # a handle that was never finalized
    h = ctypes.c_void_p()
    assert L.ff_create((str(ctx.dir / "t16b2") + ".ffplan").encode(), ctypes.byref(h)) == 0
    try:
        refused(h, ctx.img, H, W, 4, CODES8, need, "ff_finalize")
    finally:
        L.ff_destroy(h)
