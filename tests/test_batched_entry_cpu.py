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


# The pairs of entry points that share one launch body: for each of the two, the refusal its first check makes -- the return code and the
# exact text, the entry point's own name included (the shared body is handed it).  Same rule as above: host addresses, first checks only.
# P and Q stand for two distinct 16-byte aligned host addresses.
P, Q = "p", "q"
_FIRST_REFUSALS = [
    ("ff_naf_tail", (None, 64, P, 64, Q, 64, 128, 64, P, P, P, P, P, 1e-6, P, P, P, P, None),
     b"ff_naf_tail: null pointer"),
    ("ff_naf_tail_images", (P, 64, P, 64, Q, 64, 66, 64, P, 2, 33, P, P, P, P, 1e-6, P, P, P, P, None),
     b"ff_naf_tail_images: rows_per_image must be a positive multiple of 32 (got B=2 rows_per_image=33)"),
    ("ff_naf_front", (P, 64, 8, 16, 64, P, P, 1e-6, P, P, P, P, Q, 64, P, P, 1 << 20, 2, None),
     b"ff_naf_front: nterms must be 1 or 3"),
    ("ff_naf_front_images", (P, 64, 0, 8, 16, 64, P, P, 1e-6, P, P, P, P, Q, 64, P, P, 1 << 20, 3, None),
     b"ff_naf_front_images: B must be 1 .. 65535 (got 0)"),
    ("ff_token_linear_gated", (P, 192, P, 192, P, P, P, P, 0.5, Q, 192, 256, 180, 180, 6, P, P, None, 0, 2, None),
     b"ff_token_linear_gated: nterms must be 1 or 3"),
    ("ff_token_linear_gated_images", (P, 192, P, 192, P, 3, 128, P, P, 0.5, Q, 192, 384, 180, 180, 6, P, P, None, 0, 3, None),
     b"ff_token_linear_gated_images: rows_per_image must be a positive multiple of 256 and M == B * rows_per_image "
     b"(1 <= B <= 65535; got B=3 rows_per_image=128 M=384)"),
    ("ff_conv2d_bf16s_kmul_images", (P, 256, P, P, 256, 256, P, 2, 3, P, P, None, 0, Q, 256, 5, 256, 256, 3, 0, None),
     b"ff_conv2d_bf16s_kmul_images: M must be B * rows_per_image and below 2^31 (got M=5 B=2 rows_per_image=3)"),
    ("ff_conv2d_bf16s_wimages", (P, 256, P, P, 256, 256, 2, 128, P, P, None, 0, Q, 256, 256, 256, 256, 3, 0, None),
     b"ff_conv2d_bf16s_wimages: rows_per_image must be a positive multiple of 256, M == B * rows_per_image and below 2^31 "
     b"(got M=256 B=2 rows_per_image=128)"),
    ("ff_dwconv3_gate_pool", (None, 512, Q, 256, 4, 4, 256, P, P, P, P, 1 << 20, None),
     b"ff_dwconv3_gate_pool: null pointer"),
    ("ff_dwconv3_gate_pool_images", (P, 512, Q, 256, 70000, 4, 4, 256, P, P, P, P, 1 << 40, None),
     b"ff_dwconv3_gate_pool_images: B must be 1 .. 65535 (got 70000)"),
    ("ff_fft_bands", (None, 3, 64, 64, P, P, P, P, P, 16, 1.0, P, P, 1 << 20, Q, 16, 0, 3, None),
     b"ff_fft_bands: null pointer"),
    ("ff_fft_bands_images", (P, 0, 64, 64, P, P, P, P, P, 16, 1.0, P, P, 1 << 20, Q, 16, 0, 3, None),
     b"ff_fft_bands_images: expects 1 <= B <= 21845 images with 2 <= W <= 8192 and 2 <= H <= 481 or 513 <= H <= 1638 (got B=0 H=64 W=64)"),
    ("ff_pool_partials", (None, 64, 1024, 64, Q, 1 << 20, None),
     b"ff_pool_partials: bad args"),
    ("ff_pool_partials_images", (P, 64, 2, 100, 64, Q, 1 << 20, None),
     b"ff_pool_partials_images: the pixels per image must be a positive multiple of 256 (1 <= B <= 65535; got B=2 P=100)"),
]


@pytest.mark.parametrize("entry,args,text", _FIRST_REFUSALS, ids=[c[0] for c in _FIRST_REFUSALS])
def test_shared_launch_body_keeps_each_entry_points_first_refusal(L, entry, args, text):
    buf = (ctypes.c_float * 128)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    at = {P: p, Q: p + 256}
    status = getattr(L, entry)(*[at[a] if isinstance(a, str) else a for a in args])
    assert status == 1                                           # FF_ERR_ARG
    assert L.ff_last_error() == text


def test_pool_partials_split_by_image():
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    part = torch.arange(12 * 4, dtype=torch.float32).reshape(12, 4)
    pp = ops.PoolPartials(part, 3, 0.5, images=3)
    assert pp.rows_per_image == 4 and pp.images == 3
    assert ops.PoolPartials(part, 3, 0.5).rows_per_image == 12
    with pytest.raises(FFError):
        ops.PoolPartials(part, 3, 0.5, images=5)
