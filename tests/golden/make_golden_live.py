"""Fixture of the LIVE-expert training step (the reference's default train_epoch, train.py:130-250: the three frozen experts run on
every batch), generated from the IMPORTED reference (build container only; the reference's code never leaves it -- only the arrays
below are committed).  Run on the CPU:

    python tests/golden/make_golden_live.py            # B=2, 16x16 LR -> train_live_b2_16.npz + train_live_b2_16.json   (seconds)

What is run, on the reference's own modules:
    model = CompleteEnhancedFusionSR(expert_ensemble=ExpertEnsemble(...), **io.MODEL_CONFIG flags)    # _ref_import.build_reference_model
    model.train();  model.expert_ensemble.eval()
    sr = model(lr).clamp(0, 1);  loss = mean |sr - hr|;  loss.backward()
with the seeded synthetic weights of all five parts (isr2_amd.weights.synth_state_dict: hat, dat, nafnet, fusion, collab) and the
lr / hr of train_inputs.make_train_batch.  As in make_golden_train.py the two nn.MultiheadAttention modules' `dropout` attribute is
set to 0.0 on the instantiated model (no reference file is touched): dropout-on is "parity unpinned (RNG stream)".
The frozen experts are put back into eval mode on the instantiated model for the same reason: train.py:158 calls model.train() on
the whole model, which leaves HAT's stochastic depth (hat_arch.py:11-37, drop_path_rate 0.1) drawing from torch's RNG stream -- two
calls of forward_all_with_hooks on one input then differ by 0.09 in HAT's output -- and lets DAT's BatchNorms normalise with batch
statistics (0.21 away from its eval-mode output on this input).  The experts this project runs are the inference networks, the ones
the cached route's files were made with.

Stored, in make_golden_train.py's layout: sr, the loss, every BatchNorm's running statistics after the forward, and for EVERY
parameter that received a gradient its L2 norm and either the whole gradient (numel <= 8192) or 256 seeded samples; the names of
trainable parameters without gradient.  The JSON next to it records how far the reference's own two routes agree:
max |model(lr) - forward_with_precomputed(lr, *forward_all_with_hooks(lr))| in train mode."""
import os
import sys
import json
import copy

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from _ref_import import build_reference_model  # noqa: E402
from make_golden_train import put, SEED  # noqa: E402
from train_inputs import make_train_batch  # noqa: E402
from isr2_amd.weights import synth_state_dict  # noqa: E402

B, H, W, INPUT_SEED, NAME = 2, 16, 16, 561, "train_live_b2_16"


def main():
    torch.manual_seed(0)
    model, ens = build_reference_model()
    sd = synth_state_dict(SEED, parts=("hat", "dat", "nafnet", "fusion", "collab"))
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys[:5]
    live_missing = [k for k in res.missing_keys if not k.endswith("num_batches_tracked")]
    model.cross_band_attn.band_attention.dropout = 0.0
    model.collaborative.cross_attn.dropout = 0.0
    model.train()
    model.expert_ensemble.eval()                                       # see the module docstring
    d = {k: torch.from_numpy(v) for k, v in make_train_batch(INPUT_SEED, B, H, W).items()}
    lr, hr = d["lr"], d["hr"]

    # the reference's own two routes, before anything has advanced the BatchNorm buffers of `model` (a copy takes the second route)
    twin = copy.deepcopy(model)
    with torch.no_grad():
        outs, feats = twin.expert_ensemble.forward_all_with_hooks(lr)
        outs = {k: v.clone() for k, v in outs.items()}
        sr_pre = twin.forward_with_precomputed(lr, outs, feats)

    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    assert not any(n.startswith("expert_ensemble.") for n, _ in named)            # the experts are frozen
    sr_raw = model(lr)
    routes = float((sr_raw.detach() - sr_pre).abs().max())
    sr = sr_raw.clamp(0, 1)
    loss = (sr - hr).abs().mean()
    loss.backward()
    blob = {"meta": np.array(json.dumps({"B": B, "h": H, "w": W, "input_seed": INPUT_SEED, "weight_seed": SEED, "dropout": 0.0,
                                         "dead_parameters_not_in_synth": live_missing})),
            "sr": sr.detach().numpy().astype(np.float32), "losses": np.array([float(loss)], dtype=np.float64)}
    nograd = []
    for n, p in named:
        if p.grad is None:
            nograd.append(n)
        else:
            put(blob, "grad", n, p.grad)
    blob["nograd"] = np.array(json.dumps(nograd))
    for n, b in model.named_buffers():
        if n.endswith(("running_mean", "running_var", "num_batches_tracked")) and not n.startswith("expert_ensemble."):
            blob["bn/" + n] = b.detach().numpy().copy()
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **blob)
    feat_absmax = {k: float(v.abs().max()) for k, v in feats.items()}
    json.dump({"reference_routes_max_abs_dev": routes, "what": "max |model(lr) - forward_with_precomputed(lr, *forward_all_with_hooks(lr))|, model.train() with "
               "expert_ensemble.eval(), dropout 0, CPU fp32", "loss": float(loss), "feature_abs_max": feat_absmax}, open(os.path.join(HERE, NAME + ".json"), "w"), indent=1)
    print("wrote", NAME + ".npz", os.path.getsize(path) // 1024, "KiB;", len(named) - len(nograd), "gradient tensors; loss", float(loss),
          "; reference routes agree to", routes, flush=True)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("FF_THREADS", "8")))
    main()
