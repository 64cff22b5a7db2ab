"""The reference's loss schedule (configs/train_config.yaml:130-170, train.py:98-118 get_loss_stage) and the loss-weight checks of
isr2_amd.train, without a GPU.  tests/golden/loss_stages.json holds get_loss_stage(e) of the reference on its shipped YAML."""
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_loss_stage_matches_reference_schedule():
    from isr2_amd.train import LOSS_STAGES, loss_stage
    ref = json.load(open(os.path.join(HERE, "golden", "loss_stages.json")))
    assert len(LOSS_STAGES) == 3
    for r in ref:
        num, w, name = loss_stage(r["epoch"])
        assert (num, name) == (r["stage"], r["name"]), r
        assert w == r["weights"], (r["epoch"], w, r["weights"])
    assert loss_stage(80)[0] == 2 and loss_stage(79)[0] == 1 and loss_stage(10 ** 6)[0] == 3


def test_validate_loss_weights_accepts_the_yaml_stages():
    from isr2_amd.train import LOSS_STAGES, validate_loss_weights
    for st in LOSS_STAGES:
        assert validate_loss_weights(st["weights"]) == st["weights"]
    w = validate_loss_weights({"l1": 1, "edge": 0.5, "l2": 0.0, "charbonnier": 0.1, "clip": 0})
    assert w["l1"] == 1.0 and isinstance(w["l1"], float)


@pytest.mark.parametrize("bad", [{"vgg": 0.1}, {"l1": 1.0, "clip": 0.5}, {"l1": 1.0, "perceptual": 0.1}, {"l1": -0.1},
                                 {"l1": 1.0, "ssim": float("nan")}])
def test_validate_loss_weights_rejects(bad):
    from isr2_amd.lib import FFError
    from isr2_amd.train import validate_loss_weights
    with pytest.raises(FFError):
        validate_loss_weights(bad)
