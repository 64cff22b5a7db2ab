"""Host side of NAFNet's per-image entry points (no GPU): the workspace sizes, the exported tile rule of the bf16-rows GEMM, and the
argument checks that refuse a launch.  Every refusal asked for here is made before the entry point touches the device, with host
addresses: were a check to regress, these calls still could not reach a launch."""
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


@pytest.mark.parametrize("H,W,C", [(20, 40, 64), (64, 64, 128), (256, 256, 64), (7, 5, 128)])
def test_naf_front_images_workspace_is_b_times_one_image(L, H, W, C):
    one = L.ff_naf_front_workspace(H, W, C)
    assert one > 0
    for B in (1, 2, 5, 16):
        assert L.ff_naf_front_images_workspace(B, H, W, C) == B * one
    assert L.ff_naf_front_images_workspace(0, H, W, C) == -1 and L.ff_naf_front_images_workspace(-3, H, W, C) == -1
    assert L.ff_naf_front_images_workspace(2, H, W, 96) == -1


@pytest.mark.parametrize("C", [64, 256, 512, 1024])
def test_dwconv3_gate_pool_images_workspace_is_b_times_one_image(L, C):
    one = L.ff_dwconv3_gate_pool_workspace(C)
    assert one == 1024 * C
    for B in (1, 2, 5, 16):
        assert L.ff_dwconv3_gate_pool_images_workspace(B, C) == B * one
    assert L.ff_dwconv3_gate_pool_images_workspace(0, C) == -1 and L.ff_dwconv3_gate_pool_images_workspace(-1, C) == -1


def test_rows_gemm_tile_rule(L):
    # 128 x 64 tiles while the 128 x 128 grid would not fill 256 CUs, from ONE image's rows: 256 rows x 2048 columns = 32 workgroups
    assert L.ff_gemm_rows_bf16_tile(256, 2048) == 2 and L.ff_gemm_rows_bf16_tile(4096, 1024) == 2
    assert L.ff_gemm_rows_bf16_tile(4096, 2048) == 1 and L.ff_gemm_rows_bf16_tile(16384, 512) == 1 and L.ff_gemm_rows_bf16_tile(65536, 256) == 1


def test_naf_front_images_refusals(L, p):
    name = "ff_naf_front_images"
    ok = dict(x=p, g=p, b=p, w=p, b1=p, dw=p, db=p, out=p, pooled=p, work=p)
    for miss in ok:
        a = dict(ok, **{miss: None})
        _refused(L, L.ff_naf_front_images(a["x"], 64, 2, 8, 16, 64, a["g"], a["b"], 1e-6, a["w"], a["b1"], a["dw"], a["db"], a["out"], 64,
                                          a["pooled"], a["work"], 1 << 20, 3, None), name)
    for B in (0, -1, 70000):
        _refused(L, L.ff_naf_front_images(p, 64, B, 8, 16, 64, p, p, 1e-6, p, p, p, p, p, 64, p, p, 1 << 20, 3, None), name)
    _refused(L, L.ff_naf_front_images(p, 96, 2, 8, 16, 96, p, p, 1e-6, p, p, p, p, p, 96, p, p, 1 << 20, 3, None), name)       # C
    _refused(L, L.ff_naf_front_images(p, 64, 2, 8, 16, 64, p, p, 1e-6, p, p, p, p, p, 64, p, p, 2 * 64 - 1, 3, None), name)    # workspace


def test_dwconv3_gate_pool_images_refusals(L, p):
    name = "ff_dwconv3_gate_pool_images"
    ok = [p, p, p, p, p, p]
    for i in range(6):
        a = list(ok)
        a[i] = None
        _refused(L, L.ff_dwconv3_gate_pool_images(a[0], 512, a[1], 256, 2, 4, 4, 256, a[2], a[3], a[4], a[5], 1 << 20, None), name)
    for B in (0, -1, 70000):
        _refused(L, L.ff_dwconv3_gate_pool_images(p, 512, p, 256, B, 4, 4, 256, p, p, p, p, 1 << 30, None), name)
    _refused(L, L.ff_dwconv3_gate_pool_images(p, 512, p, 256, 2, 4, 4, 256, p, p, p, p, 2 * 256 - 1, None), name)             # workspace


def test_naf_tail_images_refusals(L, p):
    name = "ff_naf_tail_images"

    def call(g=p, x=p, out=None, sca=p, M=128, B=2, rpi=64, w=p):
        o = p + 256 if out is None else out
        return L.ff_naf_tail_images(g, 64, x, 64, o, 64, M, 64, sca, B, rpi, p, p, p, p, 1e-6, w, p, p, p, None)

    for kw in (dict(g=None), dict(x=None), dict(sca=None), dict(w=None)):
        _refused(L, call(**kw), name)
    for rpi in (0, 1, 16, 48, 100):                              # a wave's 32 rows must be one image's
        _refused(L, call(M=2 * rpi, rpi=rpi), name)
    _refused(L, call(M=127), name)                               # M != B * rows_per_image
    _refused(L, call(M=192), name)
    _refused(L, call(B=0, M=0), name)


def test_conv2d_bf16s_kmul_images_refusals(L, p):
    name = "ff_conv2d_bf16s_kmul_images"

    def call(inp=p, hi=p, km=p, out=p, M=8, B=2, rpi=4):
        return L.ff_conv2d_bf16s_kmul_images(inp, 256, hi, p, 256, 256, km, B, rpi, p, p, p, 256, out, 256, M, 256, 256, 3, 0, None)

    for kw in (dict(inp=None), dict(hi=None), dict(km=None), dict(out=None)):
        _refused(L, call(**kw), name)
    for kw in (dict(M=7), dict(M=9), dict(B=0, M=0), dict(rpi=0, M=0), dict(B=3, M=8)):
        _refused(L, call(**kw), name)


def test_gemm_rows_bf16_kmul_images_refusals(L, p):
    name = "ff_gemm_rows_bf16_kmul_images"

    def call(a=p, hi=p, km=p, out=p, M=8, B=2, rpi=4, K=256):
        return L.ff_gemm_rows_bf16_kmul_images(a, 256, hi, K, km, B, rpi, p, p, p, 256, out, 256, M, 256, K, 0, None)

    for kw in (dict(a=None), dict(hi=None), dict(km=None), dict(out=None)):
        _refused(L, call(**kw), name)
    for kw in (dict(M=7), dict(M=9), dict(B=0, M=0), dict(rpi=0, M=0), dict(B=3, M=8)):
        _refused(L, call(**kw), name)
    _refused(L, call(K=200), name)                               # K % 64
