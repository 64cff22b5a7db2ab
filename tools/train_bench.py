"""Time the fusion-only training step (BASELINE config 5: batch 16 x 64 x 64 LR, experts precomputed) on one MI355X.
    python tools/train_bench.py [--batch 16] [--size 64] [--steps 5] [--mode bf16x3|f32] [--loss-stage 1|2|3] [--accum A]
--accum A: every optimizer step accumulates A micro-batches of --batch samples (FusionTrainer.accumulate); ms/step is per optimizer step.
--loss-stage selects the reference's loss weights of that stage (isr2_amd.train.LOSS_STAGES; 1 = L1 only, the default); for stages
2 and 3 the loss kernels alone (forward + gradient of the 4h x 4w prediction) are timed as well.
Under rocprofv3 --kernel-trace --stats the per-kernel table of a step comes out of the same command."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", default="f32")
    ap.add_argument("--loss-stage", type=int, default=1, choices=(1, 2, 3))
    ap.add_argument("--accum", type=int, default=1)
    a = ap.parse_args()
    from train_inputs import make_train_batch
    from isr2_amd import ops
    from isr2_amd.train import FusionTrainer
    from isr2_amd.weights import synth_state_dict
    ops.set_gemm_mode(a.mode)
    d = {k: torch.from_numpy(v).cuda() for k, v in make_train_batch(503, a.batch, a.size, a.size).items()}
    outs = {k: d["out_" + k] for k in ("hat", "dat", "nafnet")}
    feats = {k: d["feat_" + k] for k in ("hat", "dat", "nafnet")}
    tr = FusionTrainer(synth_state_dict(1234, parts=("fusion", "collab")), "cuda:0", gemm=a.mode)
    if a.loss_stage != 1:
        tr.set_stage(a.loss_stage)
    window = [(d["lr"], d["hr"], outs, feats)] * a.accum

    def one():
        return tr.step(d["lr"], d["hr"], outs, feats) if a.accum == 1 else tr.accumulate(window)[-1]
    for _ in range(a.warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = one()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / a.steps
    print(f"train step B={a.batch} x accum {a.accum} {a.size}x{a.size} mode={a.mode}: {ms:.2f} ms/step, loss {float(loss):.6f}, "
          f"peak HBM {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB", flush=True)
    if a.loss_stage != 1:
        from isr2_amd import ops as _ops
        hr = _ops.nchw_to_nhwc(d["hr"])
        sr = (hr * 1.1 - 0.05).contiguous()
        dsr = torch.empty_like(sr)
        for _ in range(2):
            tr.srloss.combined(tr.active_losses, sr, hr, dsr, tr.loss_values, tr.active_w, tr.loss)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            tr.srloss.combined(tr.active_losses, sr, hr, dsr, tr.loss_values, tr.active_w, tr.loss)
        torch.cuda.synchronize()
        ms_loss = 1e3 * (time.perf_counter() - t0) / a.steps
        print(f"loss stage {a.loss_stage} {dict(tr.active_losses)}: loss kernels {ms_loss:.3f} ms per call "
              f"(prediction {tuple(sr.shape)}); components {tr.last_loss_components()}", flush=True)


if __name__ == "__main__":
    main()
