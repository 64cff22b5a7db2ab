"""Fixtures of two file contracts with the reference's training side, generated from the IMPORTED reference (build container
only; the reference's code never leaves it -- only what its code was seen to read and return is committed).

    python tests/golden/make_golden_contracts.py         # -> cache_reader_view.npz, fusion_ckpt_layout.json   (seconds)

cache_reader_view.npz -- two cached-expert samples written by isr2_amd.cache.write_sample (tests/test_cache.py::_fake_sample,
    seeds 0 and 1, 4x3 LR):
        file/<part file name>/<key path>    every entry of every part file, as written (the filename string as a 0-d str array)
        reader/len                          len(CachedSRDataset(dir, augment=False, repeat_factor=1, load_features=True))
        reader/<i>/<key path>               what its __getitem__(i) returned
    The reference's reader is checked to load these files before anything is stored.

fusion_ckpt_layout.json -- the cached-mode CompleteEnhancedFusionSR (tests/golden/make_golden_train.py::build_cached_mode_model):
        state_dict        [key, shape, dtype] in the model's own state_dict() order
        parameters        named_parameters() order (= the optimizer's parameter order and the EMA shadow's keys)
        resume_reads      keys of the checkpoint dict (and of its ema_state_dict) that CheckpointManager.load_checkpoint and
                          EMAModel.load_state_dict read when resuming from a checkpoint of isr2_amd.train.build_checkpoint
    Before it is stored, such a checkpoint is loaded through the reference's own CheckpointManager into the model, AdamW,
    CosineAnnealingWarmRestarts and EMAModel, and checked tensor by tensor.
"""
import contextlib
import importlib.util
import io as _io
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _ref_import import REF_ROOT  # noqa: E402


class _Recorder(dict):
    """A dict that notes which keys were read."""
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.read = []

    def _note(self, key):
        if key not in self.read:
            self.read.append(key)

    def __getitem__(self, key):
        self._note(key)
        return super().__getitem__(key)

    def get(self, key, default=None):
        self._note(key)
        return super().get(key, default)

    def __contains__(self, key):
        self._note(key)
        return super().__contains__(key)


def flatten(d, prefix=""):
    out = {}
    for k, v in d.items():
        p = f"{prefix}/{k}" if prefix else str(k)
        if isinstance(v, dict):
            out.update(flatten(v, p))
        elif isinstance(v, torch.Tensor):
            out[p] = v.numpy()
        else:
            out[p] = np.array(v)
    return out


def cache_reader_view(path):
    from isr2_amd import cache
    from test_cache import _fake_sample
    spec = importlib.util.spec_from_file_location("ref_cached_dataset", os.path.join(REF_ROOT, "src", "data", "cached_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    blob = {}
    with tempfile.TemporaryDirectory() as d:
        for i in range(2):
            cache.write_sample(d, f"img_{i:03d}", *_fake_sample(seed=i, h=4, w=3))
        for f in sorted(os.listdir(d)):
            blob.update(flatten(torch.load(os.path.join(d, f), weights_only=True), "file/" + f))
        with contextlib.redirect_stdout(_io.StringIO()):
            ds = mod.CachedSRDataset(d, augment=False, repeat_factor=1, load_features=True)
        assert len(ds) == 2
        blob["reader/len"] = np.array(len(ds))
        for i in range(len(ds)):
            item = ds[i]
            lr, hr, outs, feats = _fake_sample(seed=i, h=4, w=3)
            assert item["filename"] == f"img_{i:03d}" and torch.equal(item["lr"], lr) and torch.equal(item["hr"], hr)
            for k in ("hat", "dat", "nafnet"):
                assert torch.equal(item["expert_imgs"][k], outs[k][0]) and torch.equal(item["expert_feats"][k], feats[k][0])
            blob.update(flatten(item, f"reader/{i}"))
    np.savez_compressed(path, **blob)
    print(f"{path}: {len(blob)} arrays")


def fusion_ckpt_layout(path):
    from make_golden_train import build_cached_mode_model, HP
    from isr2_amd import train as TR
    with contextlib.redirect_stdout(_io.StringIO()):
        model, _, _ = build_cached_mode_model()
        from src.utils.checkpoint_manager import CheckpointManager, EMAModel
    full = model.state_dict()
    layout = {"state_dict": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in full.items()],
              "parameters": [n for n, _ in model.named_parameters()]}
    # a checkpoint of build_checkpoint, resumed by the reference exactly as train.py:943-966 does
    names = TR.trainable_names(full)
    g = torch.Generator().manual_seed(0)
    params = {k: full[k] + 0.01 * torch.randn(full[k].shape, generator=g) for k in names}
    m = {k: 0.01 * torch.randn(full[k].shape, generator=g) for k in names}
    v = {k: 1e-4 * torch.rand(full[k].shape, generator=g) for k in names}
    model_sd = type(full)((k, params.get(k, t)) for k, t in full.items())
    ema = {k: model_sd[k] * 0.5 for k in model_sd if TR.is_parameter_key(k)}
    ck = TR.build_checkpoint(model_sd, m, v, ema, step=7, hp=dict(TR.HP), epoch=3, metrics={"psnr": 30.05, "loss": 0.02}, lr_now=1.2e-4,
                             scheduler_state={"T_0": 50, "T_i": 50, "T_mult": 2, "eta_min": 5e-8, "T_cur": 3, "base_lrs": [1.5e-4], "last_epoch": 3,
                                              "_step_count": 4, "_get_lr_called_within_step": False, "_last_lr": [1.2e-4]})
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "checkpoint_epoch0003.pth")
        TR._save_atomic(ck, p)
        load = torch.load
        rec = {}

        def recording_load(*a, **k):
            rec["ck"] = _Recorder(load(*a, **k))
            return rec["ck"]
        with contextlib.redirect_stdout(_io.StringIO()):
            model2, _, _ = build_cached_mode_model()
            opt = torch.optim.AdamW(model2.parameters(), lr=HP["lr"], betas=HP["betas"], weight_decay=HP["weight_decay"], eps=HP["eps"])
            sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=50, T_mult=2, eta_min=5e-8)
            ema2 = EMAModel(model2, decay=0.999)
            torch.load = recording_load
            try:
                got = CheckpointManager(os.path.join(d, "mgr")).load_checkpoint(p, model2, opt, sched, load_optimizer=True, device="cpu")
            finally:
                torch.load = load
            ema_st = _Recorder(got["ema_state_dict"])
            ema2.load_state_dict(ema_st)
    named = dict(model2.named_parameters())
    for k in names:
        assert torch.equal(named[k].data, params[k]), k
        st = opt.state[named[k]]
        assert torch.equal(st["exp_avg"], m[k]) and torch.equal(st["exp_avg_sq"], v[k]) and float(st["step"]) == 7.0, k
    assert ema2.decay == TR.HP["ema_decay"] and len(ema2.shadow) == len(layout["parameters"])
    assert opt.param_groups[0]["lr"] == 1.2e-4 and sched.T_cur == 3
    layout["resume_reads"] = {"checkpoint": list(rec["ck"].read), "ema_state_dict": list(ema_st.read)}
    with open(path, "w") as f:                                        # one entry per line: diffs stay readable
        f.write("{\"state_dict\": [\n" + ",\n".join(json.dumps(e) for e in layout["state_dict"]) + "],\n"
                "\"parameters\": [\n" + ",\n".join(json.dumps(n) for n in layout["parameters"]) + "],\n"
                "\"resume_reads\": " + json.dumps(layout["resume_reads"]) + "}\n")
    print(f"{path}: {len(layout['state_dict'])} state-dict entries, {len(layout['parameters'])} parameters, reads {layout['resume_reads']}")


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("FF_THREADS", "8")))
    cache_reader_view(os.path.join(HERE, "cache_reader_view.npz"))
    fusion_ckpt_layout(os.path.join(HERE, "fusion_ckpt_layout.json"))
