"""ff_color_jitter_pairs (csrc/color_jitter.hip, ops.color_jitter_pairs) against the numpy restatement tests/golden/jitter_ref.py, bit for
bit (torch.equal): p in {1, 3, 4, 16, 17, 64} -- float4 and dword forms, one chunk and many (4p = 256: 64 chunks of 1024 pixels per
sample) --, B in {1, 3} with mixed apply flags, random bytes plus all-zero and all-255 patches, corner factors, factors that drive values
out of [0, 1], saturated colours whose Sat clips, sf == 1, an unaligned view."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import jitter_ref as J  # noqa: E402

F = np.float32
# {apply, bf, cf, sf}: the corners of the default ranges, a pair that leaves [0, 1] on both sides, sf == 1, nearly-one factors
ROWS = [[1, 0.8, 1.2, 1.2], [0, 0.8, 1.2, 0.8], [1, 1.2, 0.8, 0.8], [1, 1.9, 1.9, 1.2], [1, 1.1, 0.9, 1.0], [1, 1.2, 1.2, 1.0000001],
        [1, 0.8, 0.8, 1.2], [0, 1.0, 1.0, 1.0], [1, 1.0, 1.0, 1.1]]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _patches(B, p, seed):
    rng = np.random.default_rng(seed)
    lr = rng.integers(0, 256, (B, 3, p, p), dtype=np.uint8)
    hr = rng.integers(0, 256, (B, 3, 4 * p, 4 * p), dtype=np.uint8)
    return lr.astype(F) / F(255), hr.astype(F) / F(255)


def _run(lr, hr, table, offset=False):
    """-> (lr, hr) numpy after the kernel; offset: the device tensors are views one float past a 16-byte boundary."""
    from isr2_amd import ops
    table = np.asarray(table, dtype=F)
    dev = []
    for a in (lr, hr):
        if offset:
            buf = torch.zeros(a.size + 1, device="cuda", dtype=torch.float32)
            t = buf[1:].view(a.shape)
            t.copy_(torch.from_numpy(a))
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        else:
            t = torch.from_numpy(a).cuda()
        dev.append(t)
    out = ops.color_jitter_pairs(dev[0], dev[1], table)
    assert out[0] is dev[0] and out[1] is dev[1]
    return dev[0].cpu().numpy(), dev[1].cpu().numpy()


def _check(lr, hr, table, **kw):
    want = J.jitter_pairs(lr, hr, table)
    got = _run(lr, hr, table, **kw)
    again = _run(lr, hr, table, **kw)
    for name, g, a, w, src in zip(("lr", "hr"), got, again, want, (lr, hr)):
        assert torch.equal(torch.from_numpy(g), torch.from_numpy(w)), (name, float(np.abs(g - w).max()), int((g != w).sum()))
        assert g.tobytes() == a.tobytes(), name                         # two runs: equal bits
        for b, row in enumerate(np.asarray(table)):
            if row[0] == 0:
                assert g[b].tobytes() == src[b].tobytes(), (name, b)    # untouched bit for bit


@pytest.mark.parametrize("p", [1, 3, 4, 16, 17, 64])
@pytest.mark.parametrize("B", [1, 3])
def test_random_bytes_equal_the_restatement(p, B):
    _need_gpu()
    lr, hr = _patches(B, p, 100 * p + B)
    rows = [ROWS[(p + 2 * j) % len(ROWS)] for j in range(B)] if B > 1 else [ROWS[p % 3 * 2]]      # B = 3: mixed apply flags
    if B > 1:
        rows[1] = [0] + rows[1][1:]
        assert {r[0] for r in rows} == {0, 1}
    _check(lr, hr, rows)


def test_every_row_of_factors_at_p16_and_the_dword_form_at_p17():
    _need_gpu()
    for p in (16, 17):
        lr, hr = _patches(len(ROWS), p, 7 + p)
        _check(lr, hr, ROWS)


def test_an_unaligned_view_takes_the_dword_form():
    _need_gpu()
    lr, hr = _patches(3, 16, 5)
    _check(lr, hr, [ROWS[0], ROWS[1], ROWS[3]], offset=True)


def test_constant_patches_and_saturated_colours():
    _need_gpu()
    p = 4
    lr, hr = _patches(4, p, 9)
    lr[0], hr[0] = 0.0, 0.0                                             # all zero: mean 0
    lr[1], hr[1] = 1.0, 1.0                                             # all 255: bf = 1.2 leaves [0, 1], the clip brings it back
    sat = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [10, 200, 250], [3, 250, 1], [200, 100, 50], [37, 91, 12]], dtype=np.uint8)
    for t, P in ((lr, p), (hr, 4 * p)):                                 # saturated colours, every pixel: Sat * 1.2 passes 255
        px = sat[np.arange(P * P) % len(sat)].reshape(P, P, 3)
        t[2] = np.moveaxis(px, -1, 0).astype(F) / F(255)
    table = [[1, 1.2, 1.2, 1.2], [1, 1.2, 0.8, 0.8], [1, 1.0, 1.0, 1.2], [1, 1.0, 1.0, 1.0]]
    _check(lr, hr, table)
    got = _run(lr, hr, table)
    assert not got[0][0].any() and not got[1][0].any()                  # black stays black
    assert (got[0][1] == 1).all() and (got[1][1] == 1).all()            # white, brightened and clipped


def test_wrapper_refuses_bad_tables_and_shapes_before_any_launch():
    _need_gpu()
    from isr2_amd import lib as L
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    real, calls = L.load(), []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    lr, hr = torch.zeros(2, 3, 4, 4, device="cuda"), torch.zeros(2, 3, 16, 16, device="cuda")
    good = [[1, 1.0, 1.0, 1.0], [0, 1.0, 1.0, 1.0]]
    L._lib = Spy()
    try:
        for row in ([2, 1.0, 1.0, 1.0], [0.5, 1.0, 1.0, 1.0], [1, 0.0, 1.0, 1.0], [1, 1.0, 2.0, 1.0], [1, 1.0, 1.0, float("nan")],
                    [1, 1.0, float("inf"), 1.0], [1, -0.5, 1.0, 1.0]):
            with pytest.raises(FFError):
                ops.color_jitter_pairs(lr, hr, [row, good[1]])
        for table in ([good[0]], [[1, 1.0, 1.0], [0, 1.0, 1.0]]):
            with pytest.raises(FFError):
                ops.color_jitter_pairs(lr, hr, table)
        for args in ((lr, hr[:, :, :8]), (lr, torch.zeros(2, 3, 8, 8, device="cuda")), (lr[:1], hr), (lr.double(), hr), (lr[..., ::2], hr),
                     (lr.cpu(), hr)):
            with pytest.raises(FFError):
                ops.color_jitter_pairs(*args, good)
        with pytest.raises(FFError):
            ops.color_jitter_pairs(lr, hr, good, table_dev=torch.zeros(2, 4, device="cuda", dtype=torch.float64))
    finally:
        L._lib = real
    assert "ff_color_jitter_pairs" not in calls
    ops.color_jitter_pairs(lr, hr, good, table_dev=torch.tensor(good, device="cuda", dtype=torch.float32))      # the good table is taken
