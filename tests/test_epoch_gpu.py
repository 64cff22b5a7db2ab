"""Whole epochs on the GPU (isr2_amd/epoch.py, FusionTrainer's accumulation windows, csrc/augment.hip) against fixtures produced by the
IMPORTED reference (tests/golden/make_golden_epoch.py): train_epoch_cached with accumulation_steps = 2 over two epochs of five
micro-batches (the fifth is the window the reference discards), gradient_clip 0.05 so that the clip is active on the accumulated
gradient, the learning rate of epochs 5 and 6 from torch's own scheduler; the same first window with the stage-3 loss weights;
validate_epoch with EMA weights.

Bars are the ones tests/test_train_gpu.py, tests/test_train_stages_gpu.py, tests/test_cached_mode.py and tests/test_metrics.py
already hold: an accumulated gradient is a mean of per-micro-batch gradients that each meet those bars.  AdamW is almost blind to
the gradient's scale, so the parameters alone would not notice a missing 1/A: the per-tensor gradients and the pre-clip norms carry
the accumulation test."""
import hashlib
import json
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
BARS = {"f32": 1e-4, "bf16x3": 1e-3}                                   # tests/test_train_gpu.py
PARAM_BARS = {"f32": 0.05, "bf16x3": 0.5}
EVAL_BARS = {"f32": 5e-5, "bf16x3": 2e-4}                              # tests/test_cached_mode.py
EXPERTS = ("hat", "dat", "nafnet")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _batch(seed, B=2, h=16, w=16):
    from train_inputs import make_train_batch
    d = {k: torch.from_numpy(v) for k, v in make_train_batch(seed, B, h, w).items()}
    return d["lr"], d["hr"], {k: d["out_" + k] for k in EXPERTS}, {k: d["feat_" + k] for k in EXPERTS}


def _sidx(name, numel, n):
    """make_golden_train.sidx: the fixture's sample positions, a draw seeded by the tensor's name (not stored)."""
    s = int.from_bytes(hashlib.sha256(("train/" + name).encode()).digest()[:4], "little")
    return np.random.default_rng(s).integers(0, numel, size=n).astype(np.int64)


def _unpack(g, kind):
    names, cnt = json.loads(str(g[f"{kind}/names"])), g[f"{kind}/count"]
    offs = np.concatenate([[0], np.cumsum(cnt)])
    return {n: (float(g[f"{kind}/l2"][i]), g[f"{kind}/vals"][offs[i]:offs[i + 1]]) for i, n in enumerate(names)}


def _cmp(ref, name, t):
    """max |t - ref| over the stored values (the whole tensor, or its samples), max |ref|, L2 of t, L2 of the reference tensor."""
    f = t.detach().float().reshape(-1).cpu().numpy()
    l2ref, vals = ref[name]
    got = f if vals.size == f.size else f[_sidx(name, f.size, vals.size)]
    return float(np.abs(got - vals).max()), float(np.abs(vals).max()), float(np.sqrt((f.astype(np.float64) ** 2).sum())), l2ref


def _trainer(meta, mode, **kw):
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    hp = dict(meta["hp"])
    hp["betas"] = tuple(hp["betas"])
    return FusionTrainer(synth_state_dict(meta["weight_seed"], parts=("fusion", "collab")), "cuda:0", hp=hp, dropout=0.0, gemm=mode, **kw), hp


def _check_grads(tag, g, tr, grads, tol):
    gref = _unpack(g, "grad")
    assert set(gref) == set(tr.names)
    assert not (set(tr.names) & set(json.loads(str(g["nograd"]))))
    gmax = float(np.abs(g["grad/vals"]).max())
    floor = 1e-3 * gmax
    worst = {}
    for k in tr.names:
        dmax, rmax, l2, l2ref = _cmp(gref, k, grads[k])
        worst[k] = dmax / max(rmax, floor)
        assert abs(l2 - l2ref) <= 20 * tol * max(l2ref, floor), (k, l2, l2ref)
    print(tag, f"{len(worst)} gradient tensors; worst relative deviations:", sorted(worst.items(), key=lambda kv: -kv[1])[:6])
    bad = {k: v for k, v in worst.items() if not v < tol}
    assert not bad, bad


def _check_params(tag, g, tr, steps, bar, step_scale, decay):
    psd, esd = tr.state_dict(), tr.ema_shadow()
    pref, eref = _unpack(g, f"param{steps}"), _unpack(g, f"ema{steps}")
    wp, we = {}, {}
    for k in tr.names:
        dmax, rmax, *_ = _cmp(pref, k, psd[k])
        wp[k] = dmax / max(1.0, rmax)
        dmax, rmax, *_ = _cmp(eref, k, esd[k])
        we[k] = dmax / max(1.0, rmax)
    print(tag, "after", steps, "optimizer steps: worst param dev", max(wp.values()), "(", max(wp.values()) / step_scale, "of the total update ); worst EMA dev", max(we.values()))
    assert max(wp.values()) < bar * step_scale, sorted(wp.items(), key=lambda kv: -kv[1])[:5]
    assert max(we.values()) < bar * step_scale * (1 - decay) * steps + 1e-6


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_accumulated_epochs_against_reference(mode):
    """Two epochs of five micro-batches, accumulation_steps 2: losses, the first window's gradients, every window's pre-clip norm,
    BatchNorm buffers after each epoch, parameters and EMA after the four optimizer steps.
    On the parent commit forward_backward takes no window arguments; its documented recipe (two forward_backward calls, one
    optimizer_step) misses the first window's gradient by 1.19 x max|ref|."""
    _need_gpu()
    from isr2_amd import epoch as E
    g = np.load(os.path.join(GOLD, "train_accum_b2_16.npz"))
    meta = json.loads(str(g["meta"]))
    tol = BARS[mode]
    A = meta["accumulation_steps"]
    assert A == 2 and meta["hp"]["clip"] == 0.05
    tr, hp = _trainer(meta, mode)
    data = [_batch(s) for s in meta["input_seeds"]]
    seen = []

    def hook(G):                                                       # between the window's last backward and the optimizer
        seen.append((G.clone(), float(G.double().norm())))

    losses = []
    for e, epoch in enumerate(meta["epochs"]):
        lr_now = E.lr_for_epoch(epoch)
        assert abs(lr_now - meta["lr"][e]) <= 1e-12 * lr_now
        res = E.train_epoch(tr, data, epoch, A, grad_hook=hook)        # lr_now from lr_for_epoch inside
        assert res["lr"] == lr_now and res["stage"] == 1
        assert (res["micro_batches"], res["optimizer_steps"], res["discarded"]) == (5, 2, 1)
        assert abs(res["loss"] - float(np.mean(g["losses"][5 * e:5 * e + 5]))) < tol
        assert not tr.window_open
        losses += res["micro_losses"]
        worst_bn = 0.0
        for k, v in tr.buffers.items():
            ref = g[f"bn_e{epoch}/" + k]
            worst_bn = max(worst_bn, float(np.abs(v.cpu().numpy() - ref).max()) / max(1.0, float(np.abs(ref).max())))
        for k, n in tr.nbt.items():                                    # every micro-batch advances them, the discarded one too
            assert n == int(g[f"bn_e{epoch}/" + k]), (k, n, int(g[f"bn_e{epoch}/" + k]))
        print(mode, "epoch", epoch, "BatchNorm running statistics worst rel. deviation =", worst_bn)
        assert worst_bn < tol
    assert tr.step_count == 4 and len(seen) == 4                       # Adam's t counts optimizer steps, not micro-batches
    dl = np.abs(np.array(losses) - g["losses"])
    print(mode, "micro-batch losses", losses, "max |d|", float(dl.max()), "first window", float(dl[:2].max()))
    assert dl[:2].max() < tol * 0.1 and dl.max() < tol                 # unscaled, per micro-batch (train.py:359)
    norms = [n for _, n in seen]
    dn = [abs(n - r) / r for n, r in zip(norms, g["grad_norms"])]
    print(mode, "pre-clip gradient norms", norms, "ref", g["grad_norms"].tolist(), "worst rel. deviation", max(dn))
    assert norms[0] > hp["clip"]                                       # the clip is active on the accumulated gradient
    assert abs(norms[0] - float(g["grad_norms"][0])) < 10 * tol * float(g["grad_norms"][0])
    assert max(dn) < 10 * tol
    _check_grads(mode, g, tr, tr._export(seen[0][0]), tol)
    _check_params(mode, g, tr, 4, PARAM_BARS[mode], 2 * sum(meta["lr"]), hp["ema_decay"])


def test_stage3_window_against_reference():
    """The first accumulated window with the stage-3 weights at the bars of tests/test_train_stages_gpu.py (B = 2 case)."""
    _need_gpu()
    TOL, PARAM_BAR = 1e-4, 0.05
    g = np.load(os.path.join(GOLD, "train_accum_stage3_b2_16.npz"))
    meta = json.loads(str(g["meta"]))
    tr, hp = _trainer(meta, "f32", loss_weights=meta["loss_weights"])
    ref_comps = json.loads(str(g["components"]))
    for i, s in enumerate(meta["input_seeds"]):
        _, loss = tr.forward_backward(*_batch(s), zero_grad=i == 0, loss_scale=1.0 / 2, micro_index=i)
        comps = tr.last_loss_components()
        print("stage 3 micro-batch", i, "loss", float(loss), "ref", float(g["losses"][i]), comps, ref_comps[i])
        assert sorted(comps) == sorted(ref_comps[i])
        for k in comps:                                                # unweighted AND unscaled
            assert abs(comps[k] - ref_comps[i][k]) < TOL * max(1.0, abs(ref_comps[i][k])), k
        assert abs(float(loss) - float(g["losses"][i])) < TOL * 0.1
    assert tr.window_open
    _check_grads("stage3", g, tr, tr.grads(), TOL)
    tr.optimizer_step(meta["lr"][0])
    print("stage 3 pre-clip norm", tr.grad_norm(), "ref", float(g["grad_norms"][0]))
    assert abs(tr.grad_norm() - float(g["grad_norms"][0])) < 10 * TOL * float(g["grad_norms"][0])
    _check_params("stage3", g, tr, 1, PARAM_BAR, meta["lr"][0], hp["ema_decay"])


def test_one_micro_batch_window_is_todays_step_bit_for_bit():
    _need_gpu()
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    sd = synth_state_dict(1234, parts=("fusion", "collab"))
    mb = _batch(511)

    def run(kind):
        tr = FusionTrainer(sd, "cuda:0", dropout=0.1, seed=7)
        for _ in range(2):
            if kind == "step":
                loss = float(tr.step(*mb))
            elif kind == "accumulate":
                loss = tr.accumulate([mb])[0]
            else:
                _, l = tr.forward_backward(*mb, zero_grad=True, loss_scale=1.0, micro_index=0)
                tr.optimizer_step()
                loss = float(l)
        return tr.P.clone(), tr.EMA.clone(), loss
    a, b, c = run("step"), run("accumulate"), run("args")
    for o in (b, c):
        assert torch.equal(a[0], o[0]) and torch.equal(a[1], o[1]) and a[2] == o[2]


def test_micro_batches_of_one_window_draw_different_dropout_masks():
    _need_gpu()
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    sd = synth_state_dict(1234, parts=("fusion", "collab"))
    mb = _batch(512)

    def window(indices, dropout=0.1):
        tr = FusionTrainer(sd, "cuda:0", dropout=dropout, seed=7)
        for i, mi in enumerate(indices):
            tr.forward_backward(*mb, zero_grad=i == 0, loss_scale=0.5, micro_index=mi)
        return tr.G.clone()
    a, b = window((0, 1)), window((0, 1))
    assert torch.equal(a, b)                                           # counter-based masks, fixed-order reductions
    same_mask = window((0, 0))
    assert not torch.equal(a, same_mask)
    assert torch.equal(window((0, 1), 0.0), window((0, 0), 0.0))       # without dropout the index changes nothing


def _torch_d4(x, codes):
    out = []
    for b, c in enumerate(codes):
        t = x[b]
        if c & 1:
            t = torch.flip(t, dims=[-1])
        if c & 2:
            t = torch.flip(t, dims=[-2])
        if c >> 2:
            t = torch.rot90(t, k=c >> 2, dims=[-2, -1])
        out.append(t)
    return torch.stack(out).contiguous()


def _undo_d4(t, c):
    if c >> 2:
        t = torch.rot90(t, k=-(c >> 2), dims=[-2, -1])
    if c & 2:
        t = torch.flip(t, dims=[-2])
    if c & 1:
        t = torch.flip(t, dims=[-1])
    return t


def test_d4_is_torchs_flip_and_rot90():
    _need_gpu()
    from isr2_amd import lib as L
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    gen = torch.Generator().manual_seed(3)
    all16 = list(range(16))
    even = [0, 1, 2, 3, 8, 9, 10, 11] * 2
    cases = [(C, n, n, all16) for C in (3, 64, 180) for n in (16, 64, 256)]
    cases += [(C, 24, 40, even) for C in (3, 64, 180)]
    cases += [(4, 72, 72, all16), (2, 136, 200, even)]                                           # edge tiles on the 16-byte path
    cases += [(3, 18, 18, all16), (5, 70, 70, all16), (3, 10, 7, even), (2, 65, 130, even)]      # W % 4 != 0: the dword path; edge tiles
    for C, H, W, codes in cases:
        x = torch.rand((len(codes), C, H, W), generator=gen)
        got = ops.d4_nchw(x.cuda(), codes).cpu()
        assert torch.equal(got, _torch_d4(x, codes)), (C, H, W)
    # an unaligned view (a channel-offset slice of a larger buffer) takes the dword path too
    buf = torch.rand(16 * 3 * 16 * 16 + 1, generator=gen)
    x = buf[1:].view(16, 3, 16, 16)
    assert torch.equal(ops.d4_nchw(buf.cuda()[1:].view(16, 3, 16, 16), all16).cpu(), _torch_d4(x, all16))
    # odd quarter turns on a non-square batch are refused before any launch
    real, calls = L.load(), []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)
    x = torch.rand(2, 3, 24, 40).cuda()
    L._lib = Spy()
    try:
        for bad in (4, 5, 12, 15):
            with pytest.raises(FFError):
                ops.d4_nchw(x, [0, bad])
        with pytest.raises(FFError):
            ops.d4_nchw(x, [0])
    finally:
        L._lib = real
    assert "ff_d4_nchw" not in calls


def _write_cache(path, n, seed, h=16, w=16):
    from train_inputs import make_train_batch
    from isr2_amd import cache
    d = {k: torch.from_numpy(v) for k, v in make_train_batch(seed, n, h, w).items()}
    for j in range(n):
        cache.write_sample(str(path), f"img{j:03d}", d["lr"][j], d["hr"][j], {k: d["out_" + k][j:j + 1] for k in EXPERTS},
                           {k: d["feat_" + k][j:j + 1] for k in EXPERTS})
    return d


def test_augmented_micro_batch_carries_one_code_per_sample(tmp_path):
    _need_gpu()
    from isr2_amd import cache
    from isr2_amd import epoch as E
    _write_cache(tmp_path, 5, 531)
    data = E.CachedEpoch(str(tmp_path), batch_size=4, repeat_factor=3, augment=True, seed=11)
    assert len(data) == 3
    for epoch in (0, 1):
        idx, codes = data.plan(epoch)
        got = list(data.batches(epoch))
        assert len(got) == 3
        for b, (lr, hr, outs, feats) in enumerate(got):
            assert lr.is_cuda and tuple(lr.shape) == (4, 3, 16, 16) and tuple(feats["hat"].shape) == (4, 180, 16, 16)
            for j in range(4):
                s = cache.read_sample(str(tmp_path), data.stems[int(idx[b, j]) % 5])
                c = int(codes[b, j])
                assert torch.equal(_undo_d4(lr[j].cpu(), c), s["lr"]) and torch.equal(_undo_d4(hr[j].cpu(), c), s["hr"])
                for k in EXPERTS:
                    assert torch.equal(_undo_d4(outs[k][j].cpu(), c), s["expert_imgs"][k]), (k, c)
                    assert torch.equal(_undo_d4(feats[k][j].cpu(), c), s["expert_feats"][k]), (k, c)
    assert len(set(int(c) for c in np.concatenate([data.plan(e)[1].reshape(-1) for e in (0, 1)]))) > 4
    plain = E.CachedEpoch(str(tmp_path), batch_size=5, augment=False, shuffle=False)
    (lr, hr, outs, feats), = list(plain.batches(0))
    for j, stem in enumerate(plain.stems):
        assert torch.equal(lr[j].cpu(), cache.read_sample(str(tmp_path), stem)["lr"])


def _epoch_from_files(data, cdir, epoch):
    """What `data` must yield for `epoch`: ops.d4_nchw of the files, in epoch_plan's order and with its codes."""
    from isr2_amd import cache, ops
    from isr2_amd import epoch as E
    idx, codes = E.epoch_plan(len(data.stems), data.repeat, data.B, data.seed, epoch, data.augment, data.shuffle)
    want = []
    for b in range(len(idx)):
        rows = [cache.sample_fields(cache.read_sample(cdir, data.stems[int(i) % len(data.stems)])) for i in idx[b]]
        want.append({k: ops.d4_nchw(torch.stack([r[k] for r in rows]).cuda(), [int(c) for c in codes[b]]) for k in E.FIELDS})
    return want


def _same_batches(got, want):
    from isr2_amd import cache
    assert len(got) == len(want)
    for g, w in zip(got, want):
        lr, hr, outs, feats = cache.fields_batch(w)
        assert torch.equal(g[0], lr) and torch.equal(g[1], hr)
        for k in EXPERTS:
            assert torch.equal(g[2][k], outs[k]) and torch.equal(g[3][k], feats[k]), k


def test_abandoned_epoch_leaves_the_next_one_whole(tmp_path):
    """Six samples at 8x8 LR, batch 2, two staging slots: three micro-batches, so a slot is reused inside one epoch.  Epoch 0 is closed
    after its first micro-batch (a reader at work, a filled slot never uploaded); all of epoch 1 still holds the files' bits."""
    _need_gpu()
    from isr2_amd import epoch as E
    _write_cache(tmp_path, 6, 571, 8, 8)
    data = E.CachedEpoch(str(tmp_path), batch_size=2, augment=True, seed=3, prefetch=2)
    assert len(data) == 3 and data.layout["feat_nafnet"][1] == (2, 64, 8, 8) and data.layout["out_dat"][1] == (2, 3, 32, 32)
    it = data.batches(0)
    first = next(it)
    it.close()
    want0, want1 = _epoch_from_files(data, str(tmp_path), 0), _epoch_from_files(data, str(tmp_path), 1)
    _same_batches([first], want0[:1])
    assert not [t.name for t in threading.enumerate() if t.name.startswith("ff-")]
    _same_batches(list(data.batches(1)), want1)
    wide = E.CachedEpoch(str(tmp_path), batch_size=2, augment=True, seed=3, prefetch=3)
    _same_batches(list(wide.batches(1)), want1)


def test_bad_sample_reaches_the_stepping_thread(tmp_path):
    """A sample whose feat_dat has another shape, in the second micro-batch: the FFError naming the file is raised by the iteration,
    and no reader thread outlives it."""
    _need_gpu()
    from isr2_amd import cache
    from isr2_amd import epoch as E
    from isr2_amd.lib import FFError
    _write_cache(tmp_path, 6, 572, 8, 8)
    lr, hr, outs, feats = cache.fields_batch(cache.sample_fields(cache.read_sample(str(tmp_path), "img002")))
    cache.write_sample(str(tmp_path), "img002", lr, hr, outs, dict(feats, dat=torch.zeros(180, 4, 8)))
    data = E.CachedEpoch(str(tmp_path), batch_size=2, augment=False, shuffle=False, prefetch=2)
    with pytest.raises(FFError, match="img002"):                        # raised while the first micro-batch is handed out or right after it
        list(data.batches(0))
    assert not [t.name for t in threading.enumerate() if t.name.startswith("ff-")]


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_validate_against_reference(mode):
    """validate() against validate_b1_16.npz.  PSNR bound: a uniform deviation of `bar` on the [0,1] scale changes the RMSE by at most
    bar, so PSNR moves by at most 20 log10(1 + bar / rmse_ref) dB (the Y weights sum to 0.859 < 1, so it holds on the Y channel)."""
    _need_gpu()
    from isr2_amd import epoch as E
    from isr2_amd.train import FusionTrainer, to_native
    from isr2_amd.weights import synth_state_dict
    from oracle import freqfusion_oracle as O
    g = np.load(os.path.join(GOLD, "validate_b1_16.npz"))
    meta = json.loads(str(g["meta"]))
    bar = EVAL_BARS[mode]
    tr = FusionTrainer(synth_state_dict(meta["weight_seed"], parts=("fusion", "collab")), "cuda:0", dropout=0.0, gemm=mode)
    other = synth_state_dict(meta["ema_seed"], parts=("fusion", "collab"))
    assert len(tr.names) == meta["shadow_taken"]
    for k in tr.names:
        tr.EMA[tr.offs[k]:tr.offs[k] + other[k].numel()].copy_(to_native(k, other[k].float()).reshape(-1))
    lr, hr, outs, feats = _batch(meta["input_seed"])
    samples = [{"lr": lr[b], "hr": hr[b], "expert_imgs": {k: outs[k][b] for k in EXPERTS}, "expert_feats": {k: feats[k][b] for k in EXPERTS}}
               for b in range(2)]
    before = (tr.P.clone(), tr.EMA.clone(), tr.M.clone(), tr.V.clone(), {k: v.clone() for k, v in tr.buffers.items()}, dict(tr.nbt), tr.step_count)
    res = {}
    for use_ema, tag in ((True, "ema"), (False, "model")):
        r = res[tag] = E.validate(tr, samples, use_ema=use_ema, crop_border=4, test_y_channel=True, return_sr=True)
        ps, ss = [], []
        for b in range(2):
            d = float((r["sr"][b] - torch.from_numpy(g["sr_" + tag][b])).abs().max())
            print(mode, tag, "image", b, "max |sr - ref| =", d, "PSNR / SSIM", r["per_image"][b], "ref", g["per_image_" + tag][b].tolist())
            assert d < bar
            ps.append(O.metric_psnr(r["sr"][b][None], hr[b][None].clamp(0, 1), 4, True))
            ss.append(O.metric_ssim(r["sr"][b][None], hr[b][None].clamp(0, 1), 4, True))
            assert abs(r["per_image"][b][0] - ps[-1]) < 2e-4 and abs(r["per_image"][b][1] - ss[-1]) < 2e-6      # tests/test_metrics.py
        assert abs(r["psnr"] - float(np.mean(ps))) < 2e-4 and abs(r["ssim"] - float(np.mean(ss))) < 2e-6         # averaging included
        ref_psnr, ref_ssim = (float(v) for v in g["mean_" + tag])
        bound = 20 * math.log10(1 + bar / 10 ** (-ref_psnr / 20))
        print(mode, tag, "PSNR", r["psnr"], "ref", ref_psnr, "bound", bound, "SSIM", r["ssim"], "ref", ref_ssim)
        assert abs(r["psnr"] - ref_psnr) < bound
        for b in range(2):
            pb = float(g["per_image_" + tag][b][0])
            assert abs(r["per_image"][b][0] - pb) < 20 * math.log10(1 + bar / 10 ** (-pb / 20))
    assert abs(res["ema"]["psnr"] - res["model"]["psnr"]) > 0.1        # the shadow is what was evaluated
    assert float((res["ema"]["sr"][0] - res["model"]["sr"][0]).abs().max()) > 1e-2
    assert set(E.validate(tr, [], use_ema=True).items()) == {("psnr", 0.0), ("ssim", 0.0)}
    after = (tr.P, tr.EMA, tr.M, tr.V)
    assert all(torch.equal(a, b) for a, b in zip(before[:4], after))
    assert all(torch.equal(v, tr.buffers[k]) for k, v in before[4].items()) and before[5] == tr.nbt and before[6] == tr.step_count


def test_resumed_run_repeats_the_uninterrupted_one(tmp_path):
    """Two epochs (augmentation and dropout on, five micro-batches of one sample, accumulation 2: two windows and a discarded one per
    epoch) against one epoch -> save_checkpoint -> a fresh trainer's load_checkpoint -> the second epoch."""
    _need_gpu()
    from isr2_amd import epoch as E
    from isr2_amd.lib import FFError
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    cdir = tmp_path / "cache"
    _write_cache(cdir, 5, 541)
    sd = synth_state_dict(1234, parts=("fusion", "collab"))

    def data():
        return E.CachedEpoch(str(cdir), batch_size=1, augment=True, seed=5)
    a = FusionTrainer(sd, "cuda:0", dropout=0.1, seed=5)
    ra = [E.train_epoch(a, data(), e, 2) for e in (0, 1)]
    assert [r["optimizer_steps"] for r in ra] == [2, 2] and [r["discarded"] for r in ra] == [1, 1] and a.step_count == 4
    b = FusionTrainer(sd, "cuda:0", dropout=0.1, seed=5)
    rb0 = E.train_epoch(b, data(), 0, 2)
    assert rb0["micro_losses"] == ra[0]["micro_losses"]
    path = b.save_checkpoint(str(tmp_path / "e0.pth"), epoch=0, lr_now=rb0["lr"])
    ck = torch.load(path, weights_only=True)
    assert sorted(ck["ff_trainer"]) == ["dropout", "seed", "step_count"] and ck["optimizer_state_dict"]["param_groups"][0]["lr"] == rb0["lr"]
    c = FusionTrainer(synth_state_dict(99, parts=("fusion", "collab")), "cuda:0", dropout=0.0, seed=0)
    c.load_checkpoint(path)
    rc1 = E.train_epoch(c, data(), int(ck["epoch"]) + 1, 2)
    assert rc1["micro_losses"] == ra[1]["micro_losses"]
    assert torch.equal(a.P, c.P) and torch.equal(a.EMA, c.EMA) and torch.equal(a.M, c.M) and torch.equal(a.V, c.V)
    for k in a.buffers:
        assert torch.equal(a.buffers[k], c.buffers[k]), k
    assert a.nbt == c.nbt and c.step_count == 4
    # checkpoints are written at window boundaries only
    mb = _batch(511)
    c.forward_backward(*mb, zero_grad=True, loss_scale=0.5, micro_index=0)
    with pytest.raises(FFError):
        c.save_checkpoint(str(tmp_path / "open.pth"), epoch=2)
    c.discard_window()
    c.save_checkpoint(str(tmp_path / "closed.pth"), epoch=2)


def test_train_cached_command_runs_two_epochs(tmp_path):
    _need_gpu()
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    _write_cache(tmp_path / "train", 5, 551)
    _write_cache(tmp_path / "val", 2, 552)
    out = tmp_path / "run"
    cmd = [sys.executable, "-m", "isr2_amd.train_cached", "--cache", str(tmp_path / "train"), "--val-cache", str(tmp_path / "val"), "--out", str(out),
           "--epochs", "2", "--batch", "2", "--accum", "2", "--repeat", "2"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [row["epoch"] for row in rows] == [0, 1]
    for row in rows:
        assert all(math.isfinite(row[k]) for k in ("loss", "psnr", "ssim", "lr")), row
        assert row["micro_batches"] == 5 and row["optimizer_steps"] == 2 and row["discarded"] == 1 and row["stage"] == 1
    assert os.path.exists(out / "latest.pth") and os.path.exists(out / "best.pth")
    tr = FusionTrainer(synth_state_dict(99, parts=("fusion", "collab")), "cuda:0")
    ck = tr.load_checkpoint(str(out / "latest.pth"))
    assert ck["epoch"] == 1 and tr.step_count == 4 and math.isfinite(ck["metrics"]["psnr"])
    # --resume continues after the checkpoint's epoch
    r = subprocess.run(cmd[:cmd.index("--epochs")] + ["--epochs", "3", "--batch", "2", "--accum", "2", "--repeat", "2", "--resume", str(out / "latest.pth")],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [row["epoch"] for row in rows] == [2]
