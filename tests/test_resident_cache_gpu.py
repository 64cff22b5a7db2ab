"""Resident cached training on the GPU (run with -m gpu on the MI355X): ff_gather_d4_fields (csrc/gather_batch.hip, ops.gather_d4_fields)
against ops.d4_nchw per field, epoch.ResidentEpoch against epoch.CachedEpoch, validation from the pool against validation from the files,
and the --resident command.  The kernel is a permutation: every comparison is torch.equal, there is no tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "golden"))
EXPERTS = ("hat", "dat", "nafnet")
SENT = 7.25                                                             # what the gaps of an output buffer must still hold


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _make_pool(shapes, n, seed, dev, lead=0):
    """A seeded field-major pool of n samples (the gaps between fields hold seeded values too) -> (pool view, offsets).  lead: floats in
    front of the view, so that lead = 1 puts every field 4 bytes off a 16-byte boundary."""
    from isr2_amd.epoch import resident_layout
    offs, total = resident_layout(shapes, n)
    buf = torch.randn(lead + total, generator=torch.Generator().manual_seed(seed)).to(dev)
    return buf[lead:], offs


def _field(pool, offs, shapes, n, f):
    C, H, W = shapes[f]
    return pool[int(offs[f]):int(offs[f]) + n * C * H * W].view(n, C, H, W)


def _gather(pool, offs, shapes, n, desc, lead_out=0):
    """-> the F gathered fields.  The output buffer starts at SENT: whatever lies between the fields must still hold it afterwards."""
    from isr2_amd import ops
    from isr2_amd.epoch import resident_layout
    desc = np.asarray(desc, dtype=np.int32)
    B = desc.shape[0]
    ooffs, ototal = resident_layout(shapes, B)
    buf = torch.full((lead_out + ototal,), SENT, device=pool.device)
    out = buf[lead_out:]
    fields = [[int(po), int(oo), *shp] for po, oo, shp in zip(offs, ooffs, shapes)]
    views = ops.gather_d4_fields(pool, n, fields, torch.from_numpy(desc).to(pool.device), out, desc_host=desc)
    torch.cuda.synchronize()
    used = torch.zeros(lead_out + ototal, dtype=torch.bool, device=pool.device)
    for oo, (C, H, W), v in zip(ooffs, shapes, views):
        assert tuple(v.shape) == (B, C, H, W) and v.data_ptr() == out.data_ptr() + 4 * int(oo)
        used[lead_out + int(oo):lead_out + int(oo) + B * C * H * W] = True
    assert bool((buf[~used] == SENT).all()), "floats outside the output fields were written"
    return views


def _check(pool, offs, shapes, n, desc, lead_out=0):
    from isr2_amd import ops
    desc = np.asarray(desc, dtype=np.int32)
    views = _gather(pool, offs, shapes, n, desc, lead_out)
    idx, codes = torch.from_numpy(desc[:, 0].astype(np.int64)).to(pool.device), [int(c) for c in desc[:, 1]]
    for f, v in enumerate(views):
        want = ops.d4_nchw(_field(pool, offs, shapes, n, f)[idx].contiguous(), codes)
        assert torch.equal(v, want), f"field {f} {shapes[f]}"
    return views


def _desc16(n, seed):
    """All 16 codes across a batch of 16, sample indices drawn with repeats."""
    idx = np.random.default_rng(seed).integers(0, n, size=16)
    idx[3] = idx[11] = idx[0]                                           # the same sample under three codes
    return np.stack((idx, np.random.default_rng(seed + 1).permutation(16)), axis=-1)


def test_lr16_shipped_fields_one_ragged_tile_vector_form(dev):
    shapes = [(3, 16, 16)] + [(3, 64, 64)] * 4 + [(180, 16, 16)] * 2 + [(64, 16, 16)]
    pool, offs = _make_pool(shapes, 5, 1, dev)
    assert pool.data_ptr() % 16 == 0 and all(int(o) % 64 == 0 for o in offs)
    _check(pool, offs, shapes, 5, _desc16(5, 2))
    _check(pool, offs, shapes, 5, [[4, 13]])                            # B = 1
    _check(pool, offs, shapes, 5, [[2, 6]] * 3)                         # one sample, one code, three times


def test_dword_and_vector_forms_in_one_launch_and_a_field_of_one_channel(dev):
    shapes = [(3, 6, 6), (3, 24, 24), (1, 6, 6), (1, 24, 24)]         # W = 6: the dword form; W = 24: the 16-byte form; C = 1
    pool, offs = _make_pool(shapes, 7, 3, dev)
    _check(pool, offs, shapes, 7, _desc16(7, 4))


def test_two_by_two_ragged_tiles_cross_tile_borders(dev):
    shapes = [(3, 20, 20), (3, 80, 80), (2, 20, 20)]                   # 80 = 64 + 16: 2 x 2 tiles, the odd-turn LDS path across tile borders
    pool, offs = _make_pool(shapes, 4, 5, dev)
    _check(pool, offs, shapes, 4, _desc16(4, 6))
    shapes = [(2, 67, 67), (1, 130, 130)]                               # widths that are no multiple of 4: ragged dword tiles, 3 x 3 of them
    pool, offs = _make_pool(shapes, 3, 7, dev)
    _check(pool, offs, shapes, 3, _desc16(3, 8))


class _Spy:
    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        self._calls.append(name)
        return getattr(self._real, name)


def test_non_square_fields_take_even_turns_and_refuse_odd_ones_before_any_launch(dev):
    from isr2_amd import lib as L
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    shapes = [(3, 8, 12), (3, 32, 48), (2, 70, 9)]
    pool, offs = _make_pool(shapes, 4, 9, dev)
    even = [0, 1, 2, 3, 8, 9, 10, 11]
    _check(pool, offs, shapes, 4, [[i % 4, c] for i, c in enumerate(even)])
    real, calls = L.load(), []
    L._lib = _Spy(real, calls)
    try:
        for c in (4, 5, 6, 7, 12, 13, 14, 15):
            with pytest.raises(FFError, match="square"):
                _gather(pool, offs, shapes, 4, [[0, 0], [1, c]])
    finally:
        L._lib = real
    assert "ff_gather_d4_fields" not in calls                           # the launch count is unchanged
    # the kernel's own guard, for a table the host never saw: the odd-turn bit is dropped, nothing outside the pool is read
    desc = np.array([[0, 5], [3, 14]], dtype=np.int32)
    from isr2_amd.epoch import resident_layout
    ooffs, ototal = resident_layout(shapes, 2)
    out = torch.full((ototal,), SENT, device=dev)
    views = ops.gather_d4_fields(pool, 4, [[int(po), int(oo), *s] for po, oo, s in zip(offs, ooffs, shapes)], torch.from_numpy(desc).to(dev), out)
    for f, v in enumerate(views):
        assert torch.equal(v, ops.d4_nchw(_field(pool, offs, shapes, 4, f)[[0, 3]].contiguous(), [1, 10]))


def test_pool_and_output_four_bytes_off_a_16_byte_boundary_take_the_dword_form(dev):
    shapes = [(3, 16, 16), (3, 64, 64), (5, 16, 16)]
    pool, offs = _make_pool(shapes, 5, 11, dev, lead=1)
    assert pool.data_ptr() % 16 == 4
    desc = _desc16(5, 12)
    a = [v.clone() for v in _check(pool, offs, shapes, 5, desc)]                          # misaligned pool, aligned output
    b = [v.clone() for v in _check(pool, offs, shapes, 5, desc, lead_out=1)]              # both misaligned
    aligned = pool.clone()
    assert aligned.data_ptr() % 16 == 0
    c = _check(aligned, offs, shapes, 5, desc, lead_out=3)                                # aligned pool, misaligned output
    d = _check(aligned, offs, shapes, 5, desc)                                            # the 16-byte form
    for f in range(3):
        assert torch.equal(a[f], b[f]) and torch.equal(a[f], c[f]) and torch.equal(a[f], d[f])


def _torch_d4_int(x, code):
    """flip(-1), flip(-2), rot90(k) of an integer plane stack [C, H, W]: torch's own index shuffles, exact on any bit pattern."""
    if code & 1:
        x = x.flip(-1)
    if code & 2:
        x = x.flip(-2)
    return torch.rot90(x, code >> 2, (-2, -1))


def test_special_values_pass_through_bit_for_bit(dev):
    """NaN payloads (quiet and signalling, both signs), -0.0, denormals and infinities: compared through an int32 view, against torch's
    integer flips and rotations of the same bits."""
    shapes = [(3, 20, 20), (2, 72, 72), (3, 6, 6)]                      # vector form, LDS path over 2 x 2 tiles, dword form
    from isr2_amd.epoch import resident_layout
    n = 3
    offs, total = resident_layout(shapes, n)
    g = torch.Generator().manual_seed(13)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (total,), generator=g, dtype=torch.int64).to(torch.int32)    # any bit pattern at all
    special = torch.tensor([0x7FC00001, 0x7F800001, -0x00400000 + 5, -0x007FFFFF, 0x7FFFFFFF, -1,             # NaNs with payloads
                            -2 ** 31, 0, 1, 0x007FFFFF, -2 ** 31 + 1, -2 ** 31 + 0x00400000,                   # -0, 0, denormals
                            0x7F800000, -0x00800000], dtype=torch.int64).to(torch.int32)                       # +inf, -inf
    pos = torch.randperm(total, generator=g)[:total // 2]
    bits[pos] = special[torch.arange(pos.numel()) % special.numel()]
    pool = bits.view(torch.float32).to(dev)
    assert torch.equal(pool.view(torch.int32).cpu(), bits)              # the upload itself keeps the bits
    f32 = pool.cpu()
    assert bool(f32.isnan().any()) and bool(((f32 == 0) & (pool.view(torch.int32).cpu() < 0)).any()) and bool(((f32.abs() > 0) & (f32.abs() < 1e-38)).any())
    desc = _desc16(n, 14)
    views = _gather(pool, offs, shapes, n, desc)
    for f, v in enumerate(views):
        src = _field(pool, offs, shapes, n, f).view(torch.int32).cpu()
        got = v.contiguous().view(torch.int32).cpu()
        for b in range(16):
            assert torch.equal(got[b], _torch_d4_int(src[int(desc[b, 0])], int(desc[b, 1]))), (f, b)


def test_wrapper_refuses_before_any_launch(dev):
    from isr2_amd import lib as L
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    shapes = [(3, 16, 16), (3, 64, 64)]
    pool, offs = _make_pool(shapes, 4, 15, dev)
    B = 2
    out = torch.zeros(B * (768 + 12288), device=dev)
    fields = [[0, 0, 3, 16, 16], [int(offs[1]), B * 768, 3, 64, 64]]
    good = np.array([[0, 3], [3, 12]], dtype=np.int32)
    gd = torch.from_numpy(good).to(dev)
    real, calls = L.load(), []
    L._lib = _Spy(real, calls)
    try:
        for bad in ([[4, 0], [0, 0]], [[-1, 0], [0, 0]], [[0, 16], [0, 0]], [[0, -1], [0, 0]], [[0, 0]], [[0, 0, 0], [0, 0, 0]]):
            with pytest.raises(FFError):
                ops.gather_d4_fields(pool, 4, fields, gd, out, desc_host=np.array(bad, dtype=np.int32))
        for args in ((pool, 4, fields, gd.long(), out), (pool, 4, fields, gd.cpu(), out), (pool, 4, fields, gd.view(-1), out),
                     (pool, 4, fields, gd[:0], out), (pool, 0, fields, gd, out), (pool, 5, fields, gd, out), (pool, 4, fields, gd, out[:-1]),
                     (pool, 4, [], gd, out), (pool, 4, [fields[0]] * 9, gd, out), (pool, 4, [f[:4] for f in fields], gd, out),
                     (pool, 4, [fields[0], [int(offs[1]), B * 768 - 1, 3, 64, 64]], gd, out),                      # output fields overlap
                     (pool, 4, [[0, 0, 3, 0, 16]], gd, out), (pool, 4, [[-64, 0, 3, 16, 16]], gd, out), (pool, 4, [[0, -4, 3, 16, 16]], gd, out),
                     (pool.double(), 4, fields, gd, out), (pool.view(2, -1), 4, fields, gd, out), (pool, 4, fields, gd, out.view(2, -1)),
                     (pool.cpu(), 4, fields, gd, out)):
            with pytest.raises(FFError):
                ops.gather_d4_fields(*args)
    finally:
        L._lib = real
    assert "ff_gather_d4_fields" not in calls
    views = ops.gather_d4_fields(pool, 4, fields, gd, out, desc_host=good)                # what the bad calls were made from is fine
    assert torch.equal(views[1], ops.d4_nchw(_field(pool, offs, shapes, 4, 1)[[0, 3]].contiguous(), [3, 12]))


def test_last_sample_starts_past_2_to_the_31_elements(dev):
    """One field of 8194 samples of [64, 64, 64] (2^18 floats each): the last one starts at element 8193 * 2^18 = 2^31 + 2^18 of an
    uninitialised 8.6 GB pool.  Only the first and the last sample are written; both are gathered."""
    from isr2_amd import ops
    n, shp = 8194, (64, 64, 64)
    per = shp[0] * shp[1] * shp[2]
    try:
        pool = torch.empty(n * per, device=dev, dtype=torch.float32)
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"the device refused the {4 * n * per} byte pool: {str(e).splitlines()[0]}")
    try:
        g = torch.Generator().manual_seed(17)
        first, last = torch.randn(shp, generator=g).to(dev), torch.randn(shp, generator=g).to(dev)
        assert (n - 1) * per > 2 ** 31
        pool[:per].copy_(first.view(-1))
        pool[(n - 1) * per:].copy_(last.view(-1))
        desc = np.array([[n - 1, 13], [0, 6], [n - 1, 3]], dtype=np.int32)
        out = torch.full((3 * per,), SENT, device=dev)
        v, = ops.gather_d4_fields(pool, n, [[0, 0, *shp]], torch.from_numpy(desc).to(dev), out, desc_host=desc)
        torch.cuda.synchronize()
        want = ops.d4_nchw(torch.stack((last, first, last)), [13, 6, 3])
        assert torch.equal(v, want)
    except RuntimeError as e:                                           # a device fault ends the session: nothing more is launched after it
        if any(w in str(e) for w in ("HIP error", "hipError", "illegal memory access", "hardware exception")):
            pytest.exit(f"GPU fault in the 2^31 gather: {e}", returncode=3)
        raise
    finally:
        pool = out = v = None
        torch.cuda.empty_cache()


# ---- the classes -------------------------------------------------------------------------------------------------------------------------
def _write_cache(path, n, seed, h=16, w=16, first=0):
    from train_inputs import make_train_batch
    from isr2_amd import cache
    d = {k: torch.from_numpy(v) for k, v in make_train_batch(seed, n, h, w).items()}
    for j in range(n):
        cache.write_sample(str(path), f"img{first + j:03d}", d["lr"][j], d["hr"][j], {k: d["out_" + k][j:j + 1] for k in EXPERTS},
                           {k: d["feat_" + k][j:j + 1] for k in EXPERTS})


@pytest.fixture(scope="module")
def cache5(dev, tmp_path_factory):
    """The temporary cache of 5 stems at 16x16 and its resident pool, shared by the tests below (never written)."""
    from isr2_amd import epoch as E
    path = tmp_path_factory.mktemp("resident") / "train"
    _write_cache(path, 5, 571)
    return str(path), E.ResidentCache(str(path), readers=3)


def test_pool_holds_the_files(cache5):
    from isr2_amd import cache
    from isr2_amd import epoch as E
    path, pool = cache5
    assert len(pool) == 5 and pool.load_s > 0 and pool.buf.numel() == pool.total_floats and pool.total_bytes == 4 * pool.total_floats
    assert pool.shapes["lr"] == (3, 16, 16) and pool.shapes["out_dat"] == (3, 64, 64) and pool.shapes["feat_nafnet"] == (64, 16, 16)
    for i, (a, b) in enumerate(zip(pool.samples(), E.read_samples(path))):
        assert a["filename"] == b["filename"] == pool.stems[i]
        assert a["lr"].is_cuda and a["lr"].data_ptr() == pool.field("lr")[i].data_ptr()               # a view of the pool
        assert torch.equal(a["lr"].cpu(), b["lr"]) and torch.equal(a["hr"].cpu(), b["hr"])
        for k in EXPERTS:
            assert a["expert_imgs"][k].shape == b["expert_imgs"][k].shape and torch.equal(a["expert_imgs"][k].cpu(), b["expert_imgs"][k])
            assert a["expert_feats"][k].shape == b["expert_feats"][k].shape and torch.equal(a["expert_feats"][k].cpu(), b["expert_feats"][k])
    assert sorted(cache.list_stems(path)) == pool.stems


@pytest.mark.parametrize("augment,shuffle", [(True, True), (False, False)])
def test_resident_epoch_yields_cached_epochs_batches(cache5, augment, shuffle):
    from isr2_amd import epoch as E
    from isr2_amd import lib as L
    path, pool = cache5
    ref = E.CachedEpoch(path, batch_size=4, repeat_factor=3, augment=augment, seed=11, shuffle=shuffle)
    data = E.ResidentEpoch(pool, batch_size=4, repeat_factor=3, augment=augment, seed=11, shuffle=shuffle)
    assert len(data) == len(ref) == 3 and data.stems == ref.stems
    seen = set()
    for epoch in (0, 1):
        want = [(lr.clone(), hr.clone(), {k: v.clone() for k, v in o.items()}, {k: v.clone() for k, v in f.items()})
                for lr, hr, o, f in ref.batches(epoch)]
        real, calls = L.load(), []
        L._lib = _Spy(real, calls)
        try:
            got = list(data.batches(epoch))
        finally:
            L._lib = real
        assert [c for c in calls if c.startswith("ff_") and c != "ff_last_error"] == ["ff_gather_d4_fields"] * 3      # one launch per micro-batch
        assert len(got) == len(want) == 3
        for (lr, hr, o, f), (lr0, hr0, o0, f0) in zip(got, want):
            assert lr.is_cuda and tuple(lr.shape) == (4, 3, 16, 16) and tuple(f["hat"].shape) == (4, 180, 16, 16)
            assert torch.equal(lr, lr0) and torch.equal(hr, hr0)
            for k in EXPERTS:
                assert torch.equal(o[k], o0[k]) and torch.equal(f[k], f0[k]), k
            assert all(t.is_contiguous() for t in (lr, hr, *o.values(), *f.values()))
        seen |= set(int(c) for c in data.plan(epoch)[1].reshape(-1))
    assert data.wait_s == 0.0
    assert (len(seen) > 4) if augment else seen == {0}


def test_validation_from_the_pool_is_validation_from_the_files(cache5):
    from isr2_amd import epoch as E
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    path, pool = cache5
    tr = FusionTrainer(synth_state_dict(1234, parts=("fusion", "collab")), "cuda:0", dropout=0.0)
    a = E.validate(tr, pool.samples(), return_sr=True)
    b = E.validate(tr, E.read_samples(path), return_sr=True)
    assert a["psnr"] == b["psnr"] and a["ssim"] == b["ssim"] and a["per_image"] == b["per_image"] and len(a["sr"]) == len(b["sr"]) == 5
    for x, y in zip(a["sr"], b["sr"]):
        assert torch.equal(x, y)


def test_refusals(dev, tmp_path):
    from isr2_amd import epoch as E
    from isr2_amd.lib import FFError
    mixed = tmp_path / "mixed"
    _write_cache(mixed, 3, 581)
    _write_cache(mixed, 1, 582, 8, 8, first=3)                          # img003: another shape
    need = 4 * E.resident_layout([(3, 16, 16)] + [(3, 64, 64)] * 4 + [(180, 16, 16)] * 2 + [(64, 16, 16)], 4)[1]
    before = torch.cuda.memory_allocated()
    with pytest.raises(FFError, match=str(need)):                       # over the cap: the bytes needed are named, nothing is allocated
        E.ResidentCache(str(mixed), max_bytes=need - 1)
    assert torch.cuda.memory_allocated() == before
    with pytest.raises(FFError, match="img003"):                        # the file is named
        E.ResidentCache(str(mixed), readers=2)
    rect = tmp_path / "rect"
    _write_cache(rect, 3, 583, 8, 12)
    pool = E.ResidentCache(str(rect), readers=2)
    with pytest.raises(FFError, match="square"):                        # odd quarter turns need square planes: refused in the constructor
        E.ResidentEpoch(pool, 2, augment=True)
    with pytest.raises(FFError):                                        # drop_last: 3 samples do not fill a batch of 4
        E.ResidentEpoch(pool, 4, augment=False)
    (lr, hr, o, f), = list(E.ResidentEpoch(pool, 3, augment=False, shuffle=False).batches(0))
    (lr0, hr0, o0, f0), = list(E.CachedEpoch(str(rect), 3, augment=False, shuffle=False).batches(0))
    assert tuple(lr.shape) == (3, 3, 8, 12) and torch.equal(lr, lr0) and torch.equal(hr, hr0) and torch.equal(f["dat"], f0["dat"])


def test_train_cached_resident_command_runs_two_epochs(dev, tmp_path):
    _write_cache(tmp_path / "train", 5, 551)
    _write_cache(tmp_path / "val", 2, 552)
    out = tmp_path / "run"
    cmd = [sys.executable, "-m", "isr2_amd.train_cached", "--cache", str(tmp_path / "train"), "--val-cache", str(tmp_path / "val"), "--out", str(out),
           "--epochs", "2", "--batch", "2", "--accum", "2", "--repeat", "2", "--resident", "--readers", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [row["epoch"] for row in rows] == [0, 1]
    for row in rows:
        assert row["data_wait_s"] == 0.0 and row["micro_batches"] == 5 and row["optimizer_steps"] == 2 and np.isfinite(row["loss"]) and np.isfinite(row["psnr"])
    assert os.path.exists(out / "latest.pth")
