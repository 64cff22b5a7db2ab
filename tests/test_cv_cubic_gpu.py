"""ff_resize_cv_cubic (csrc/resample.hip, ops.resize_cv_cubic) against the numpy restatement tests/golden/cv_cubic_ref.py, bit for bit
(torch.equal): up and down at non-integer ratios, the identity, the 16-byte and the scalar store forms, an unaligned output, one plane
and six, inputs far outside [0, 1] (nothing is clamped); refusals that make no launch."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import cv_cubic_ref as R  # noqa: E402

F = np.float32
# (Hi, Wi, Ho, Wo)
SHAPES = [(1, 1, 3, 2), (2, 3, 5, 7), (9, 7, 2, 3), (40, 24, 16, 9), (33, 21, 33, 21), (5, 8, 20, 32), (5, 8, 20, 31)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _input(planes, Hi, Wi, seed):
    """[N, C, Hi, Wi] with N * C == planes: values in about [-6, 7], far outside [0, 1]."""
    rng = np.random.default_rng(seed)
    n, c = (2, 3) if planes == 6 else (1, planes)
    return (rng.standard_normal((n, c, Hi, Wi)) * 2 + 0.5).astype(F)


@pytest.mark.parametrize("planes", [1, 6])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_equals_the_restatement(shape, planes):
    _need_gpu()
    from isr2_amd import ops
    Hi, Wi, Ho, Wo = shape
    x = _input(planes, Hi, Wi, 1000 * Hi + 10 * Wo + planes)
    want = R.resize32(x, Ho, Wo)
    got = ops.resize_cv_cubic(torch.from_numpy(x).cuda(), Ho, Wo)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    g = got.cpu()
    assert torch.equal(g, torch.from_numpy(want)), (float((g - torch.from_numpy(want)).abs().max()), int((g != torch.from_numpy(want)).sum()))
    assert float(g.min()) < 0 or float(g.max()) > 1 or planes == 1     # nothing was clamped
    if (Hi, Wi) == (Ho, Wo):
        assert g.numpy().tobytes() == x.tobytes()                       # the identity, bit for bit
    again = ops.resize_cv_cubic(torch.from_numpy(x).cuda(), Ho, Wo)
    assert torch.equal(again, got)


@pytest.mark.parametrize("planes", [1, 6])
def test_an_unaligned_output_takes_the_scalar_stores(planes):
    """Wo % 4 == 0 but the output starts one float past a 16-byte boundary; the floats around it stay untouched."""
    _need_gpu()
    from isr2_amd import ops
    Hi, Wi, Ho, Wo = 5, 8, 20, 32
    x = _input(planes, Hi, Wi, 77 + planes)
    n, c = x.shape[:2]
    buf = torch.full((n * c * Ho * Wo + 2,), -123.0, device="cuda", dtype=torch.float32)
    out = buf[1:-1].view(n, c, Ho, Wo)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    ret = ops.resize_cv_cubic(torch.from_numpy(x).cuda(), Ho, Wo, out=out)
    assert ret is out
    assert torch.equal(out.cpu(), torch.from_numpy(R.resize32(x, Ho, Wo)))
    assert float(buf[0]) == -123.0 and float(buf[-1]) == -123.0
    aligned = ops.resize_cv_cubic(torch.from_numpy(x).cuda(), Ho, Wo)
    assert aligned.data_ptr() % 16 == 0 and torch.equal(aligned, out)  # the 16-byte form writes the same bits


def test_a_wrong_table_gives_wrong_values_not_a_fault():
    """Indices far outside the image are clamped inside the kernel: the result is the restatement's with the clamped table."""
    _need_gpu()
    from isr2_amd import ops
    Hi, Wi, Ho, Wo = 9, 7, 4, 6
    x = _input(1, Hi, Wi, 5)
    xd = torch.from_numpy(x).cuda()
    (iw, ww), (ih, wh) = R.tables(Wi, Wo), R.tables(Hi, Ho)
    bad_w, bad_h = iw.copy(), ih.copy()
    bad_w[0], bad_w[-1], bad_h[1], bad_h[-1] = -(1 << 30), (1 << 30), (1 << 31) - 1, -(1 << 31)
    dev = lambda a: torch.from_numpy(a).cuda()                          # noqa: E731
    got = ops.resize_cv_cubic(xd, Ho, Wo, tables=((dev(bad_w), dev(ww)), (dev(bad_h), dev(wh)))).cpu().numpy()
    cw, ch = np.clip(bad_w, 0, Wi - 1), np.clip(bad_h, 0, Hi - 1)
    v = x[..., :, cw]
    h = ((v[..., 0] * ww[:, 0] + v[..., 1] * ww[:, 1]) + v[..., 2] * ww[:, 2]) + v[..., 3] * ww[:, 3]
    r = np.moveaxis(h[..., ch, :], -2, -1)
    want = ((r[..., 0] * wh[:, 0, None] + r[..., 1] * wh[:, 1, None]) + r[..., 2] * wh[:, 2, None]) + r[..., 3] * wh[:, 3, None]
    assert got.tobytes() == want.astype(F).tobytes()


def test_refusals_make_no_launch():
    _need_gpu()
    from isr2_amd import lib as L
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    real, calls = L.load(), []
    Hi, Wi, Ho, Wo = 5, 8, 6, 4
    x = torch.from_numpy(_input(1, Hi, Wi, 3)).cuda()
    out = torch.full((1, 1, Ho, Wo), -7.0, device="cuda")
    (iw, ww), (ih, wh) = (tuple(torch.from_numpy(a).cuda() for a in R.tables(n, m)) for n, m in ((Wi, Wo), (Hi, Ho)))
    # the C entry point: null pointers and non-positive sizes return an error before any launch
    ptrs = [x.data_ptr(), out.data_ptr(), 1, Hi, Wi, Ho, Wo, iw.data_ptr(), ww.data_ptr(), ih.data_ptr(), wh.data_ptr(), None]
    for pos in (0, 1, 7, 8, 9, 10):
        args = list(ptrs)
        args[pos] = None
        assert real.ff_resize_cv_cubic(*args) != 0 and b"ff_resize_cv_cubic" in real.ff_last_error()
    for pos in (2, 3, 4, 5, 6):
        for bad in (0, -1, (1 << 20) + 1):
            args = list(ptrs)
            args[pos] = bad
            assert real.ff_resize_cv_cubic(*args) != 0 and b"ff_resize_cv_cubic" in real.ff_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    L._lib = Spy()
    try:
        good = ((iw, ww), (ih, wh))
        for tables in (((iw[:-1], ww), (ih, wh)), ((iw, ww[:-1]), (ih, wh)), ((iw, ww), (ih[:-1], wh)), ((iw, ww), (ih, torch.cat([wh, wh]))),
                       ((ih, wh), (iw, ww)), ((iw.long(), ww), (ih, wh)), ((iw, ww.double()), (ih, wh)), ((iw.cpu(), ww), (ih, wh)),
                       ((iw, ww), (ih, wh[:, :3])), ((iw, ww),), (iw, ww, ih, wh), ((iw.t().contiguous().t(), ww), (ih, wh))):
            with pytest.raises(FFError):
                ops.resize_cv_cubic(x, Ho, Wo, out=out, tables=tables)
        for size in ((0, 4), (4, 0), (-3, 4)):
            with pytest.raises(FFError):
                ops.resize_cv_cubic(x, *size)
        for bad_x in (x[0], x.double(), x.cpu(), x[..., ::2], x[:0]):
            with pytest.raises(FFError):
                ops.resize_cv_cubic(bad_x, Ho, Wo)
        for bad_out in (out[..., :3], out.double(), torch.empty(1, 1, Ho + 1, Wo, device="cuda"), out.cpu()):
            with pytest.raises(FFError):
                ops.resize_cv_cubic(x, Ho, Wo, out=bad_out)
        assert "ff_resize_cv_cubic" not in calls
        ops.resize_cv_cubic(x, Ho, Wo, out=out, tables=good)            # the good tables are taken
        assert calls.count("ff_resize_cv_cubic") == 1
    finally:
        L._lib = real
    assert torch.equal(out.cpu(), torch.from_numpy(R.resize32(x.cpu().numpy(), Ho, Wo)))
