"""The live-expert training step against the IMPORTED reference (tests/golden/make_golden_live.py -> train_live_b2_16.npz): the
reference's model(lr) in train mode -- its own experts, then the fusion stack -- clamp, L1, backward; here
model.experts_with_features(lr) -> FusionTrainer.forward_backward.  Dropout 0 and the experts as inference networks on both sides
(see the generator's docstring); the reference's two routes then agree to the number in train_live_b2_16.json (0.0).

Bars: the ones tests/test_train_gpu.py applies to the trainer's f32 mode -- the fusion step is the same code -- for the forward output,
the loss, the BatchNorm statistics and every gradient tensor.  What is new here is the deviation of the HIP experts from the
reference's (the fixture of test_train_gpu.py feeds both sides the same expert tensors): f32 experts and bf16x3 experts, each in
front of the f32 trainer."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
TOL = 1e-4                                                             # tests/test_train_gpu.py BARS["f32"]: the trainer runs in f32
EXPERTS = ("hat", "dat", "nafnet")


def _cmp(g, prefix, name, t):
    f = t.detach().float().reshape(-1).cpu().numpy()
    if f"{prefix}/{name}/full" in g.files:
        ref, got = g[f"{prefix}/{name}/full"], f
    else:
        ref, got = g[f"{prefix}/{name}/val"], f[g[f"{prefix}/{name}/idx"]]
    l2 = float(np.sqrt((f.astype(np.float64) ** 2).sum()))
    return float(np.abs(got - ref).max()), float(np.abs(ref).max()), l2, float(g[f"{prefix}/{name}/l2"])


@pytest.fixture(scope="module")
def golden():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from train_inputs import make_train_batch
    g = np.load(os.path.join(GOLD, "train_live_b2_16.npz"))
    meta = json.loads(str(g["meta"]))
    d = {k: torch.from_numpy(v) for k, v in make_train_batch(meta["input_seed"], meta["B"], meta["h"], meta["w"]).items()}
    routes = json.load(open(os.path.join(GOLD, "train_live_b2_16.json")))
    assert routes["reference_routes_max_abs_dev"] <= 1e-6              # the reference's own routes agree: one target, not two
    return g, meta, d["lr"], d["hr"]


@pytest.mark.parametrize("expert_mode", ["f32", "bf16x3"])
def test_live_step_against_reference(golden, expert_mode):
    from isr2_amd import ops
    from isr2_amd.model import FreqFusionHIP
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    g, meta, lr, hr = golden
    old = ops.gemm_mode()
    ops.set_gemm_mode(expert_mode)
    try:
        model = FreqFusionHIP(synth_state_dict(meta["weight_seed"]), "cuda:0")
        outs, feats = model.experts_with_features(lr.cuda())
    finally:
        ops.set_gemm_mode(old)
    assert set(outs) == set(feats) == set(EXPERTS)
    tr = FusionTrainer(synth_state_dict(meta["weight_seed"], parts=("fusion", "collab")), "cuda:0", dropout=0.0, gemm="f32")
    nograd = set(json.loads(str(g["nograd"])))
    ref_names = {k.split("/", 1)[1].rsplit("/", 1)[0] for k in g.files if k.startswith("grad/")}
    assert set(tr.names) == ref_names and not (set(tr.names) & nograd)
    sr, loss = tr.forward_backward(lr, hr, outs, feats)
    dsr = float((ops.nhwc_to_nchw(sr).cpu() - torch.from_numpy(g["sr"])).abs().max())
    dloss = abs(float(loss) - float(g["losses"][0]))
    worst_bn = 0.0
    for k, v in tr.buffers.items():
        ref = g["bn/" + k]
        worst_bn = max(worst_bn, float(np.abs(v.cpu().numpy() - ref).max()) / max(1.0, float(np.abs(ref).max())))
    grads = tr.grads()
    gmax = max(float(np.abs(g[k]).max()) for k in g.files if k.startswith("grad/") and k.endswith(("/full", "/val")))
    floor = 1e-3 * gmax
    worst, worst_l2 = {}, {}
    for k in tr.names:
        dmax, rmax, l2, l2ref = _cmp(g, "grad", k, grads[k])
        worst[k] = dmax / max(rmax, floor)
        worst_l2[k] = abs(l2 - l2ref) / max(l2ref, floor)
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:6]
    print(f"live step, {expert_mode} experts + f32 trainer: train-mode forward max|d| = {dsr:.3e}, |loss - ref| = {dloss:.3e} (loss {float(loss):.7f}), "
          f"BatchNorm statistics worst rel. deviation = {worst_bn:.3e}, {len(worst)} gradient tensors: worst relative deviation "
          f"{max(worst.values()):.3e}, worst L2 deviation {max(worst_l2.values()):.3e}; worst six: {top}")
    assert dsr < TOL
    assert dloss < TOL * 0.1
    for k, n in tr.nbt.items():
        assert n == int(g["bn/" + k]), (k, n)
    assert worst_bn < TOL
    assert max(worst_l2.values()) <= 20 * TOL, sorted(worst_l2.items(), key=lambda kv: -kv[1])[:5]
    bad = {k: v for k, v in worst.items() if not v < TOL}
    assert not bad, bad
