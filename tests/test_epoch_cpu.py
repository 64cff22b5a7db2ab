"""Host logic of the epoch driver (isr2_amd/epoch.py): the learning-rate schedule against torch's own scheduler driven in the
reference's loop order (tests/golden/lr_schedule.json, make_golden_epoch.py), the epoch plan, the accumulation windows, metric
averaging.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def test_lr_for_epoch_matches_the_driven_scheduler():
    from isr2_amd.epoch import lr_for_epoch
    g = json.load(open(os.path.join(GOLD, "lr_schedule.json")))
    ref = g["lr"]
    assert len(ref) == 400
    for e, r in enumerate(ref):
        assert abs(lr_for_epoch(e, **g["config"]) - r) <= 1e-12 * r, (e, lr_for_epoch(e), r)
        assert abs(lr_for_epoch(e) - r) <= 1e-12 * r                  # the defaults ARE the shipped configuration
    # the loop's quirks: epoch 5 still runs at epoch 4's warm-up value, the cosine starts at epoch 6, the first restart is epoch 55
    assert lr_for_epoch(5) == lr_for_epoch(4) and abs(lr_for_epoch(4) - 1.2010e-4) < 1e-9
    assert abs(lr_for_epoch(6) - 1.4985e-4) < 1e-8
    assert lr_for_epoch(54) < 3e-7 and lr_for_epoch(55) == 1.5e-4
    assert lr_for_epoch(0) == 5e-7
    assert lr_for_epoch(0, warmup_epochs=0) == 1.5e-4 and lr_for_epoch(1, warmup_epochs=0) < 1.5e-4


def test_epoch_plan_visits_every_index_at_most_once_and_is_keyed_by_seed_and_epoch():
    from isr2_amd.epoch import epoch_plan
    idx, codes = epoch_plan(5, 3, 4, seed=7, epoch=2)
    assert idx.shape == (3, 4) and codes.shape == (3, 4)               # 15 entries, batch 4, drop_last
    flat = idx.reshape(-1)
    assert len(set(flat.tolist())) == flat.size and flat.min() >= 0 and flat.max() < 15
    assert codes.min() >= 0 and codes.max() < 16
    idx2, codes2 = epoch_plan(5, 3, 4, seed=7, epoch=2)
    assert np.array_equal(idx, idx2) and np.array_equal(codes, codes2)
    idx3, codes3 = epoch_plan(5, 3, 4, seed=7, epoch=3)
    assert not np.array_equal(idx, idx3) and not np.array_equal(codes, codes3)
    idx4, _ = epoch_plan(5, 3, 4, seed=8, epoch=2)
    assert not np.array_equal(idx, idx4)
    _, c0 = epoch_plan(5, 3, 4, seed=7, epoch=2, augment=False)
    assert not c0.any()
    big_i, big_c = epoch_plan(100, 20, 14, seed=0, epoch=0)
    assert big_i.shape == (2000 // 14, 14) and len(set(big_i.reshape(-1).tolist())) == big_i.size
    assert set(big_c.reshape(-1).tolist()) == set(range(16))           # all eight symmetries, both encodings of each
    from isr2_amd.lib import FFError
    with pytest.raises(FFError):
        epoch_plan(0, 1, 4, 0, 0)


def test_window_plan_with_an_odd_number_of_micro_batches():
    from isr2_amd.epoch import window_plan
    plan, discarded = window_plan(5, 2)
    assert discarded == 1
    assert [w["zero_grad"] for w in plan] == [True, False, True, False, True]
    assert [w["step"] for w in plan] == [False, True, False, True, False]
    assert [w["micro_index"] for w in plan] == [0, 1, 0, 1, 0]
    assert all(w["loss_scale"] == 0.5 for w in plan)
    plan, discarded = window_plan(3, 1)                                # today's step: zero, scale 1, micro 0, step -- every time
    assert discarded == 0 and all(w == dict(zero_grad=True, loss_scale=1.0, micro_index=0, step=True) for w in plan)
    plan, discarded = window_plan(2, 3)
    assert discarded == 2 and not any(w["step"] for w in plan)
    from isr2_amd.lib import FFError
    with pytest.raises(FFError):
        window_plan(4, 0)


def test_mean_metrics_skips_infinite_psnr_only():
    from isr2_amd.epoch import mean_metrics
    m = mean_metrics([float("inf"), 30.0, 20.0], [1.0, 0.5, 0.3])
    assert m["psnr"] == 25.0 and abs(m["ssim"] - 0.6) < 1e-12
    assert mean_metrics([], []) == {"psnr": 0.0, "ssim": 0.0}
    assert mean_metrics([float("inf")], [1.0]) == {"psnr": 0.0, "ssim": 1.0}
    assert all(math.isfinite(v) for v in m.values())


def test_d4_codes_are_checked_on_the_host():
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    assert ops.d4_check_codes(range(16), 64, 64) == list(range(16))
    assert ops.d4_check_codes([0, 1, 2, 3, 8, 9, 10, 11], 24, 40) == [0, 1, 2, 3, 8, 9, 10, 11]      # even k
    for bad in (4, 7, 12, 15):
        with pytest.raises(FFError):
            ops.d4_check_codes([0, bad], 24, 40)
    with pytest.raises(FFError):
        ops.d4_check_codes([16], 8, 8)


class _FakeTrainer:
    """Records what train_epoch asks of a trainer (host logic only; tensors on the CPU)."""

    def __init__(self):
        import torch
        self.calls, self.hp, self._default_loss, self.window_open = [], {"lr": 1.5e-4}, True, False
        self.G, self.n = torch.zeros(4), 0

    def set_epoch(self, epoch):
        self.calls.append(("set_epoch", epoch))
        return 1

    def discard_window(self):
        self.calls.append(("discard",))

    def forward_backward(self, lr, hr, outs, feats, *, zero_grad=True, loss_scale=1.0, micro_index=0):
        import torch
        self.calls.append(("fb", zero_grad, loss_scale, micro_index))
        self.n += 1
        return None, torch.tensor([float(self.n)])

    def optimizer_step(self, lr_now=None):
        self.calls.append(("opt", lr_now))


def test_train_epoch_drives_windows_and_discards_the_incomplete_one():
    from isr2_amd.epoch import train_epoch, lr_for_epoch
    tr, hooks = _FakeTrainer(), []
    res = train_epoch(tr, [(None, None, None, None)] * 5, 6, accumulation_steps=2, grad_hook=lambda g: hooks.append(len(tr.calls)))
    lr6 = lr_for_epoch(6)
    assert tr.calls == [("set_epoch", 6), ("discard",),
                        ("fb", True, 0.5, 0), ("fb", False, 0.5, 1), ("opt", lr6),
                        ("fb", True, 0.5, 0), ("fb", False, 0.5, 1), ("opt", lr6),
                        ("fb", True, 0.5, 0), ("discard",)]
    assert hooks == [4, 7]                                             # the all-reduce hook: once per window, before the optimizer
    assert (res["micro_batches"], res["optimizer_steps"], res["discarded"], res["stage"], res["lr"]) == (5, 2, 1, 1, lr6)
    assert res["micro_losses"] == [1.0, 2.0, 3.0, 4.0, 5.0] and res["loss"] == 3.0 and res["l1"] == 3.0      # mean over ALL micro-batches
    tr = _FakeTrainer()
    res = train_epoch(tr, [(None, None, None, None)] * 2, 0, accumulation_steps=1, lr_now=1e-3)
    assert tr.calls[2:] == [("fb", True, 1.0, 0), ("opt", 1e-3), ("fb", True, 1.0, 0), ("opt", 1e-3)] and res["discarded"] == 0
    assert train_epoch(_FakeTrainer(), [], 0, 2)["loss"] == 0.0
