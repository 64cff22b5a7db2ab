"""Host side of the per-image entry points (no GPU): the partial-row count of the batched 3x3 convolution, the exported implicit-GEMM
tile rule, the argument checks that refuse a launch, and PoolPartials' per-image row count."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def L():
    from isr2_amd import lib
    return lib.load()


@pytest.mark.parametrize("H,W,Cout,bn,nterms", [(32, 48, 180, 192, 3), (37, 45, 180, 192, 1), (64, 64, 60, 64, 1), (64, 64, 60, 64, 3),
                                                (256, 256, 60, 64, 1), (64, 64, 32, 32, 1)])
def test_images_pool_rows_are_b_times_one_image(L, H, W, Cout, bn, nterms):
    one = L.ff_conv3x3_halo_pool_rows(1, H, W, Cout, bn, nterms)
    assert one > 0
    for B in (1, 2, 5, 16):
        assert L.ff_conv3x3_halo_images_pool_rows(B, H, W, Cout, bn, nterms) == B * one
    assert L.ff_conv3x3_halo_images_pool_rows(0, H, W, Cout, bn, nterms) == -1
    assert L.ff_conv3x3_halo_images_pool_rows(2, H, W, Cout, 100, nterms) == -1


def test_whole_launch_form_depends_on_batch_but_images_form_does_not(L):
    # 64 x 64 x 60 channels, plain bf16, bn 32: one image is 16 tiles (8-row small-grid form, 32 partial rows); 32 images are 512 tiles,
    # where the whole-launch entry switches to 16-row workgroups -- the images entry keeps one image's form
    one = L.ff_conv3x3_halo_pool_rows(1, 64, 64, 32, 32, 1)
    assert one == 32
    assert L.ff_conv3x3_halo_pool_rows(32, 64, 64, 32, 32, 1) == 32 * 16
    assert L.ff_conv3x3_halo_images_pool_rows(32, 64, 64, 32, 32, 1) == 32 * one


def test_igemm_tile_rule(L):
    # the only M-dependent branch: 256 x 192 tiles from 16 384 rows on (HAT's 180-channel 3x3 convolutions below 1 024 pixels per image)
    assert L.ff_conv2d_bf16s_tile(768, 180, 1620, 1) == 5 and L.ff_conv2d_bf16s_tile(16383, 180, 1620, 1) == 5 and L.ff_conv2d_bf16s_tile(16384, 180, 1620, 1) == 4
    assert L.ff_conv2d_bf16s_tile(768, 180, 180, 1) == 7 and L.ff_conv2d_bf16s_tile(16384, 180, 180, 1) == 4
    assert L.ff_conv2d_bf16s_tile(16384, 180, 27, 0) == 7                                                     # no 16-byte loads: never the 256 x 192 tile
    assert L.ff_conv2d_bf16s_tile(1 << 20, 24, 64, 1) == 3 and L.ff_conv2d_bf16s_tile(256, 64, 64, 1) == 7
    assert L.ff_conv2d_bf16s_tile(256, 256, 576, 1) == 5 and L.ff_conv2d_bf16s_tile(1 << 20, 256, 576, 1) == 5


# Only refusals that the FIRST check of an entry point makes are asked for here, with host addresses: were a later check to regress, these
# calls still could not reach a launch.  The later checks are exercised on device buffers (tests/test_batched_ops_gpu.py).
def test_token_projmlp_images_refuses_bad_geometry_before_the_launch(L):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    for B, rpi, M in ((3, 128, 384), (0, 256, 0), (3, 0, 0), (3, 257, 771), (70000, 256, 70000 * 256)):
        assert L.ff_token_projmlp_images(p, 192, p, 192, p, 192, p, 180, B, rpi, p, 192, M, 180, 12, p, p, p, p, 1e-5, p, p, p, 3, 0, None) == 1, (B, rpi, M)
        assert b"ff_token_projmlp_images" in L.ff_last_error()          # FF_ERR_ARG: an image is whole 256-token workgroups


def test_pool_vec_mlp_images_refuses_null_pointers(L):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for part, w1, w2, out in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.ff_pool_vec_mlp_images(part, 2, 6, 192, 1.0, 180, w1, p, 6, 2, w2, p, 180, 4, 1.0, out, None, None) == 1


def test_pool_partials_split_by_image():
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    part = torch.arange(12 * 4, dtype=torch.float32).reshape(12, 4)
    pp = ops.PoolPartials(part, 3, 0.5, images=3)
    assert pp.rows_per_image == 4 and pp.images == 3
    assert ops.PoolPartials(part, 3, 0.5).rows_per_image == 12
    with pytest.raises(FFError):
        ops.PoolPartials(part, 3, 0.5, images=5)
