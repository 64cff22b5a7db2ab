"""Tiled C executor on the GPU: ff_tile_cut_u8 / ff_tile_ramps / ff_tile_finish_u8 against the ops they replace, and
ff_forward_image_u8 (a [2,3,16,16] tile plan, uint8 in and out) against the plugin's own _tiled_forward.  torch.equal throughout."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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
    img = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[0, 0, 0], img[-1, -1, 2], img[H // 2, W // 2, 1] = 0, 255, 255
    return torch.from_numpy(img).cuda()


# ---- the three kernels ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def img37(L):
    from isr2_amd import ops
    img = _image(11, 37, 29)
    assert int(img.min()) == 0 and int(img.max()) == 255
    return img, ops.u8_to_f32_image(img)


@pytest.mark.parametrize("y,x,th,tw", [(0, 0, 16, 16), (21, 13, 16, 16), (5, 1, 16, 16), (5, 2, 16, 16), (5, 3, 16, 16), (5, 4, 16, 16), (5, 20, 32, 8)])
def test_tile_cut_equals_convert_then_slice(L, img37, y, x, th, tw):
    """37x29 image; (21, 13) is the tile flush to the bottom-right corner, the last a tall 32-row, 8-column tile."""
    img, full = img37
    H, W, _ = img.shape
    out = torch.full((1, 3, th, tw), -1.0, device="cuda")
    assert L.ff_tile_cut_u8(img.data_ptr(), H, W, y, x, th, tw, out.data_ptr(), _stream()) == 0, L.ff_last_error()
    assert torch.equal(out, full[..., y:y + th, x:x + tw])


def test_tile_cut_row_starts_cover_all_byte_alignments_and_a_wide_tile(L):
    from isr2_amd import ops
    W = 29
    assert {3 * (y * W + x) % 4 for y, x in ((0, 0), (21, 13), (5, 1), (5, 2), (5, 3), (5, 4))} == {0, 1, 2, 3}   # (5, 4) brings 3
    img = _image(12, 19, 40)                                       # an 8x32 tile (wider than tall) needs a 40-wide image
    full = ops.u8_to_f32_image(img)
    out = torch.full((1, 3, 8, 32), -1.0, device="cuda")
    assert L.ff_tile_cut_u8(img.data_ptr(), 19, 40, 11, 7, 8, 32, out.data_ptr(), _stream()) == 0, L.ff_last_error()
    assert torch.equal(out, full[..., 11:19, 7:39])
    keep = out.clone()
    assert L.ff_tile_cut_u8(img.data_ptr(), 19, 40, 12, 7, 8, 32, out.data_ptr(), _stream()) != 0     # one row too low
    assert b"leaves the 19x40 image" in L.ff_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, keep)


@pytest.mark.parametrize("st,blend", [(64, 16), (64, 1), (64, 2), (64, 0), (512, 128)])
def test_tile_ramps_equal_the_plugins_table(L, st, blend):
    import models.team29_FreqFusion.io as plug
    want = plug._ramp_table(st, blend, torch.device("cuda:0"))
    tab = torch.full((4, st), -1.0, device="cuda")
    assert L.ff_tile_ramps(tab.data_ptr(), st, blend, _stream()) == 0, L.ff_last_error()
    assert torch.equal(tab, want)
    if blend > 1:
        assert float(tab[1, blend - 1]) == 1.0 and float(tab[2, -1]) == 0.0 and float(tab[1, 0]) == 0.0


@pytest.mark.parametrize("H,W,shift", [(1, 1, 0), (3, 5, 0), (64, 68, 0), (64, 68, 1)])
def test_tile_finish_equals_normalize_then_convert(L, H, W, shift):
    """shift = 1: the destination starts one byte past a 4-byte boundary (the scalar path); 3x5: 15 pixels, three vector groups and
    a tail of three, the planes 60 bytes apart (dword-aligned vector loads only)."""
    from isr2_amd import ops
    rng = np.random.default_rng(100 * H + W)
    wsum = torch.from_numpy(rng.choice(np.array([0.0, 0.25, 1.0, 2.0], dtype=np.float32), size=(1, 1, H, W))).cuda()
    if H * W >= 4:
        wsum.view(-1)[:4] = torch.tensor([0.0, 0.25, 1.0, 2.0], device="cuda")
    acc = torch.from_numpy(rng.uniform(-0.2, 1.3, (1, 3, H, W)).astype(np.float32)).cuda() * wsum
    acc0 = acc.clone()
    want_f = acc.clone()
    ops.tile_normalize(want_f, wsum)
    want = ops.f32_to_u8_image(want_f)
    buf = torch.full((3 * H * W + 8,), 0xA5, device="cuda", dtype=torch.uint8)
    assert buf.data_ptr() % 4 == 0
    out = buf[shift:shift + 3 * H * W]
    assert L.ff_tile_finish_u8(acc.data_ptr(), wsum.data_ptr(), H, W, out.data_ptr(), _stream()) == 0, L.ff_last_error()
    assert torch.equal(out.view(H, W, 3), want)
    assert torch.equal(acc, acc0), "ff_tile_finish_u8 must leave acc untouched"
    assert bool((buf[:shift] == 0xA5).all()) and bool((buf[shift + 3 * H * W:] == 0xA5).all()), "bytes outside the image were written"
    if H * W >= 64:
        assert int(want.min()) == 0 and int(want.max()) == 255     # both clamps are hit


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
    c.dir = tmp_path_factory.mktemp("tileplan_" + request.param)
    c.pair = torch.from_numpy(np.random.default_rng(21).random((BATCH, 3, TILE, TILE), dtype=np.float32)).cuda()
    stem = str(c.dir / "t16b2")
    c.info = plan.export_plan(c.model, c.pair, stem)
    c.nat = plan.NativeModel(stem + ".ffplan", stem + ".ffwts")
    c.img = _image(31, 37, 29)
    try:
        yield c
    finally:
        c.nat.close()
        _drop_graphs(c.model)
        ops.set_gemm_mode(prev)


def _work_views(work, H, W):
    """acc [1,3,4H,4W] and wsum [1,1,4H,4W] of the layout include/ff_kernels.h states: acc at 0, wsum at the next multiple of 256."""
    P = 16 * H * W
    acc = work[:12 * P].view(torch.float32).view(1, 3, 4 * H, 4 * W)
    o = _a256(12 * P)
    wsum = work[o:o + 4 * P].view(torch.float32).view(1, 1, 4 * H, 4 * W)
    return acc, wsum


def _expected_bytes(H, W):
    return _a256(12 * 16 * H * W) + _a256(4 * 16 * H * W) + _a256(12 * BATCH * TILE * TILE) + _a256(12 * BATCH * 16 * TILE * TILE) + _a256(16 * 4 * TILE)


@pytest.mark.parametrize("overlap,ntiles", [(4, 9), (6, 12)])
def test_image_through_the_tile_plan_equals_the_plugins_tiled_forward(ctx, overlap, ntiles):
    """37x29 through [2,3,16,16]: overlap 4 -> 3x3 tiles (odd: the last group is padded with a repeat), overlap 6 -> 4x3 tiles and
    blend = min(24, 16), the capped branch.  The plugin runs single-tile forwards; uint8 AND the fp32 canvas must be equal."""
    import models.team29_FreqFusion.io as plug
    from isr2_amd import ops
    assert ops.gemm_mode() == ctx.mode
    H, W, _ = ctx.img.shape
    step = TILE - overlap
    assert len(plug._tile_positions(H, TILE, step)) * len(plug._tile_positions(W, TILE, step)) == ntiles
    assert (4 * overlap > 4 * TILE // 4) == (overlap == 6)             # 16 = 16 at overlap 4, 24 capped to 16 at overlap 6
    lr = ops.u8_to_f32_image(ctx.img)
    want_f = plug._tiled_forward(ctx.model, lr, TILE, overlap, 4, torch.device("cuda:0")).clone()
    want = ops.f32_to_u8_image(want_f)
    need = ctx.nat.image_workspace_bytes(H, W)
    assert need == _expected_bytes(H, W)
    work = torch.full((need,), 0xFF, device="cuda", dtype=torch.uint8)      # NaN bit patterns: nothing may be read before it is written
    got = ctx.nat.forward_image_u8(ctx.img, overlap=overlap, work=work)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4 * H, 4 * W, 3)
    assert torch.equal(got, want), f"{int((got != want).sum())} bytes differ"
    acc, wsum = _work_views(work, H, W)
    canvas = acc.clone()
    ops.tile_normalize(canvas, wsum)
    assert torch.equal(canvas, want_f), "the fp32 canvas differs from _tiled_forward"
    # the default work buffer and a second call on a dirty one
    assert torch.equal(ctx.nat.forward_image_u8(ctx.img, overlap=overlap), want)
    assert torch.equal(ctx.nat.forward_image_u8(ctx.img, overlap=overlap, work=work), want)


def test_image_of_one_tile_equals_the_batched_forward(ctx):
    from isr2_amd import ops
    img = _image(32, TILE, TILE)
    lr = ops.u8_to_f32_image(img)
    pair = torch.cat([lr, lr])
    want = ops.f32_to_u8_image(ctx.nat(pair)[0:1])
    got = ctx.nat.forward_image_u8(img, overlap=4)
    assert torch.equal(got, want)
    assert torch.equal(want, ops.f32_to_u8_image(ctx.model(lr)))


def test_image_call_is_graph_capturable(ctx):
    H, W, _ = ctx.img.shape
    want = ctx.nat.forward_image_u8(ctx.img, overlap=4)
    work = torch.empty(ctx.nat.image_workspace_bytes(H, W), device="cuda", dtype=torch.uint8)
    static_in = ctx.img.clone()
    static_out = torch.zeros_like(want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = ctx.L.ff_forward_image_u8(ctx.nat.h, static_in.data_ptr(), H, W, 4, static_out.data_ptr(), work.data_ptr(), work.numel(), _stream())
    assert rc == 0, ctx.L.ff_last_error()
    for _ in range(2):
        static_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, want)
    del g


def test_image_call_refusals_name_the_sizes_and_write_nothing(ctx, tmp_path):
    from isr2_amd import plan
    from isr2_amd.lib import FFError
    L, nat = ctx.L, ctx.nat
    H, W, _ = ctx.img.shape
    need = nat.image_workspace_bytes(H, W)
    work = torch.empty(need, device="cuda", dtype=torch.uint8)
    out = torch.full((4 * 40, 4 * 40, 3), 0x5A, device="cuda", dtype=torch.uint8)

    def refused(handle, img, h, w, overlap, nbytes, *words):
        rc = L.ff_forward_image_u8(handle, img.data_ptr(), h, w, overlap, out.data_ptr(), work.data_ptr(), nbytes, _stream())
        err = L.ff_last_error().decode()
        assert rc != 0 and "ff_forward_image_u8" in err, err
        for wd in words:
            assert wd in err, (wd, err)
        torch.cuda.synchronize()
        assert bool((out == 0x5A).all()), "a refused call wrote to out"

    small = _image(33, 15, 40)
    refused(nat.h, small, 15, 40, 4, need, "15x40", "16x16", "ragged")
    refused(nat.h, ctx.img, H, W, 16, need, "overlap 16", "16")
    refused(nat.h, ctx.img, H, W, -1, need, "overlap -1")
    refused(nat.h, ctx.img, H, W, 4, need - 1, "37x29", str(need), str(need - 1))
    with pytest.raises(FFError, match="15x40"):
        nat.forward_image_u8(small, overlap=4)
    with pytest.raises(FFError, match="15x40"):
        nat.image_workspace_bytes(15, 40)
    with pytest.raises(FFError, match="overlap 16"):
        nat.forward_image_u8(ctx.img, overlap=16)
    with pytest.raises(FFError, match=str(need - 1)):
        nat.forward_image_u8(ctx.img, overlap=4, work=work[:need - 1])
    with pytest.raises(FFError):
        nat.forward_image_u8(ctx.img.float())

    # a plan with a non-square tile is no tile plan
    stem = str(tmp_path / "t16x24")
    lr = torch.from_numpy(np.random.default_rng(22).random((1, 3, 16, 24), dtype=np.float32)).cuda()
    plan.export_plan(ctx.model, lr, stem, verify=False)
    rect = plan.NativeModel(stem + ".ffplan", stem + ".ffwts")
    try:
        refused(rect.h, ctx.img, H, W, 4, need, "[1,3,16,24]", "[1,3,64,96]")
        with pytest.raises(FFError, match=r"\[1,3,16,24\]"):
            rect.forward_image_u8(ctx.img, overlap=4)
        with pytest.raises(FFError, match=r"\[1,3,16,24\]"):
            rect.image_workspace_bytes(H, W)
    finally:
        rect.close()
    # a handle that was never finalized
    h = ctypes.c_void_p()
    assert L.ff_create((str(ctx.dir / "t16b2") + ".ffplan").encode(), ctypes.byref(h)) == 0
    try:
        refused(h, ctx.img, H, W, 4, need, "ff_finalize")
    finally:
        L.ff_destroy(h)
