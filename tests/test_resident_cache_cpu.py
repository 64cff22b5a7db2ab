"""The host side of resident cached training, without a GPU: the pool layout (epoch.resident_layout), the size cap of
epoch.ResidentCache (refused before anything is allocated), the first check of ff_gather_d4_fields (csrc/gather_batch.hip) through
ctypes, and ResidentEpoch's plan, which is epoch_plan -- CachedEpoch's."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
EXPERTS = ("hat", "dat", "nafnet")


def _shipped(p=64):
    return [(3, p, p)] + [(3, 4 * p, 4 * p)] * 4 + [(180, p, p)] * 2 + [(64, p, p)]


def test_resident_layout_offsets_alignment_and_totals():
    from isr2_amd.epoch import FIELDS, resident_layout
    from isr2_amd.lib import FFError
    assert FIELDS == ("lr", "hr", "out_hat", "out_dat", "out_nafnet", "feat_hat", "feat_dat", "feat_nafnet")
    shapes = _shipped()
    per = [c * h * w for c, h, w in shapes]
    assert sum(per) == 2535424                                          # one sample at the shipped patch size: 10.14 MB
    for n in (1, 5, 4000):
        offs, total = resident_layout(shapes, n)
        assert offs.dtype == np.int64 and offs.shape == (8,) and offs[0] == 0
        # every shipped field is a multiple of 64 floats per sample: the fields are back to back
        assert [int(o) for o in offs] == [n * sum(per[:f]) for f in range(8)] and total == n * sum(per)
    # DF2K at five crops: 3450 images x 5 = 17250 samples, 4.4e10 floats -- past 2^31, still exact (Python / int64 arithmetic)
    offs, total = resident_layout(shapes, 17250)
    assert total == 17250 * 2535424 and total > 2 ** 35 and int(offs[-1]) == 17250 * sum(per[:7])
    # odd shapes: each field starts on the next multiple of 64 floats, the total is the end of the last field (no padding after it)
    odd = [(3, 6, 6), (3, 24, 24), (1, 5, 7), (2, 8, 12)]
    for n in (1, 3, 7):
        offs, total = resident_layout(odd, n)
        end = 0
        for f, (c, h, w) in enumerate(odd):
            assert int(offs[f]) % 64 == 0 and end <= int(offs[f]) < end + 64
            end = int(offs[f]) + n * c * h * w
        assert total == end
    offs, total = resident_layout(odd, 3)
    assert [int(o) for o in offs] == [0, 384, 5568, 5696] and total == 5696 + 3 * 2 * 8 * 12
    for bad in (([], 3), (odd, 0), ([(3, 0, 4)], 1), ([(3, 4)], 1), ([(3, 4, -1)], 2)):
        with pytest.raises(FFError):
            resident_layout(*bad)


def _write_cache(path, n, seed, h=16, w=16):
    from train_inputs import make_train_batch
    from isr2_amd import cache
    d = {k: torch.from_numpy(v) for k, v in make_train_batch(seed, n, h, w).items()}
    for j in range(n):
        cache.write_sample(str(path), f"img{j:03d}", d["lr"][j], d["hr"][j], {k: d["out_" + k][j:j + 1] for k in EXPERTS},
                           {k: d["feat_" + k][j:j + 1] for k in EXPERTS})


def test_cap_is_refused_before_anything_is_allocated(tmp_path, monkeypatch):
    from isr2_amd import epoch as E
    from isr2_amd.lib import FFError
    _write_cache(tmp_path, 2, 561, 8, 8)
    need = 4 * E.resident_layout([(3, 8, 8)] + [(3, 32, 32)] * 4 + [(180, 8, 8)] * 2 + [(64, 8, 8)], 2)[1]
    made = []
    real_empty = torch.empty

    def spy(*a, **k):                                                   # the pool (a device tensor) and the pinned slots; torch.load's own
        if k.get("pin_memory") or torch.device(k.get("device") or "cpu").type != "cpu":        # small host tensors are not the point
            made.append((a, k))
        return real_empty(*a, **k)
    monkeypatch.setattr(torch, "empty", spy)
    with pytest.raises(FFError, match=str(need)) as ei:
        E.ResidentCache(str(tmp_path), max_bytes=need - 1)
    assert "max_bytes" in str(ei.value) and not made                    # neither the pool nor a pinned slot was asked for
    with pytest.raises(FFError):
        E.ResidentCache(str(tmp_path), readers=0)
    empty = tmp_path / "none"
    empty.mkdir()
    with pytest.raises(FFError):
        E.ResidentCache(str(empty))


def test_gather_entry_refuses_bad_arguments_without_a_gpu():
    from isr2_amd import lib as L
    lib = L.load()
    assert lib.ff_abi_version() == 7

    def call(pool=16, n=4, rows=((0, 0, 3, 8, 8),), F=None, desc=16, B=2, out=16):
        if rows is None:
            return lib.ff_gather_d4_fields(pool, n, None, F, desc, B, out, None)
        fl = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 5))
        return lib.ff_gather_d4_fields(pool, n, fl.ctypes.data, len(fl) if F is None else F, desc, B, out, None)

    ok = (0, 0, 3, 8, 8)
    # 16 = a non-null dummy address: nothing is dereferenced or launched by a refused call
    bad = [dict(pool=None), dict(desc=None), dict(out=None), dict(rows=None, F=1), dict(B=0), dict(B=-1), dict(F=0),
           dict(rows=(ok,) * 9), dict(rows=(ok,) * 9, F=9), dict(n=0), dict(n=-3),
           dict(rows=((0, 0, 0, 8, 8),)), dict(rows=((0, 0, 3, 0, 8),)), dict(rows=((0, 0, 3, 8, 0),)), dict(rows=((0, 0, 3, -8, 8),)),
           dict(rows=((0, 0, -1, 8, 8),)), dict(rows=(ok, (64, 64, 3, 8, -2))),
           dict(rows=((-1, 0, 3, 8, 8),)), dict(rows=((0, -64, 3, 8, 8),)), dict(rows=(ok, (-64, 0, 3, 8, 8))),
           dict(rows=((0, 0, 2 ** 20, 2 ** 12, 2 ** 12),), B=2 ** 11)]                             # 2^43 tiles: past the grid limit
    for kw in bad:
        assert call(**kw) != 0 and b"ff_gather_d4_fields" in lib.ff_last_error(), kw


def test_gather_wrapper_refuses_cpu_tensors():
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    with pytest.raises(FFError):
        ops.gather_d4_fields(torch.zeros(4 * 192), 4, [[0, 0, 3, 8, 8]], torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2 * 192))


def test_resident_epoch_plan_is_cached_epochs_plan():
    """Both are epoch_plan: neither constructor is needed to say so, but the methods are what a run calls."""
    from isr2_amd import epoch as E

    class Pool:                                                         # what ResidentEpoch reads of a ResidentCache
        stems, dev, dir = [f"s{i}" for i in range(5)], torch.device("cpu"), "none"
        shapes = dict(zip(E.FIELDS, _shipped(16)))
        offsets = E.resident_layout(_shipped(16), 5)[0]

    for aug, shuf in ((True, True), (False, False), (True, False)):
        res = E.ResidentEpoch(Pool(), 4, 3, augment=aug, seed=11, shuffle=shuf)
        ce = E.CachedEpoch.__new__(E.CachedEpoch)
        ce.stems, ce.repeat, ce.B, ce.seed, ce.augment, ce.shuffle = Pool.stems, 3, 4, 11, aug, shuf
        assert len(res) == len(ce) == 3 and res.wait_s == 0.0
        for e in (0, 1, 7):
            (i0, c0), (i1, c1), (i2, c2) = res.plan(e), ce.plan(e), E.epoch_plan(5, 3, 4, 11, e, aug, shuf)
            assert np.array_equal(i0, i1) and np.array_equal(c0, c1) and np.array_equal(i0, i2) and np.array_equal(c0, c2)
            d = res.descriptors(e)
            assert d.dtype == np.int32 and d.shape == (3, 4, 2) and np.array_equal(d[..., 0], i0 % 5) and np.array_equal(d[..., 1], c0)
    # the gather table: pool offsets, batch offsets (the layout of B samples), shapes
    assert res.fields.shape == (8, 5) and np.array_equal(res.fields[:, 0], Pool.offsets)
    assert np.array_equal(res.fields[:, 1], E.resident_layout(_shipped(16), 4)[0]) and res.out_floats == E.resident_layout(_shipped(16), 4)[1]
    from isr2_amd.lib import FFError
    with pytest.raises(FFError):                                        # drop_last: too few samples for one batch
        E.ResidentEpoch(Pool(), 16, 3)
    with pytest.raises(FFError):
        E.ResidentEpoch(Pool(), 0)

    class Rect(Pool):
        shapes = dict(Pool.shapes, lr=(3, 8, 12))
    with pytest.raises(FFError, match="square"):                        # odd quarter turns need square planes: refused in the constructor
        E.ResidentEpoch(Rect(), 4, 3, augment=True)
    E.ResidentEpoch(Rect(), 4, 3, augment=False)
