"""The call table of the whole-image path at BASELINE config 4 (GPU tool, run once on the MI355X).

    python tests/golden/make_bigextent_calls.py [out.json]          # default: tests/golden/bigextent_calls.json

Wraps the public functions of isr2_amd.ops from the outside (ops.py is not edited), runs one whole-image forward of the
2040x1356 LR image of tests/test_plugin_gpu.py::test_config4_image_through_the_plugin in each of bf16x3, bf16 and f32, and
writes one row per distinct (op, kernel route, mode, operand role, pitch, channels, rows) of every call in which some operand
spans rows * ld >= 2^30 elements.  `call` names the launch the operand belongs to (op, route, mode, the scalar arguments that
select a kernel form, the small tensor arguments that are present, and the shapes [dtype, ld, channels, rows] of the large operands),
so the rows of one launch can be put together again; `ge31` / `ge32` mark extents at or past
2^31 / 2^32 elements.  The route is the one ops chose: re-derived from the arguments the way ops.conv2d / ops.linear /
ff_resize decide, and cross-checked against the prepared weight images (PREPARED.of) after the call.
Only recorded results are written; tests/test_bigextent_*.py read them.
"""
import inspect
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)

from isr2_amd import ops  # noqa: E402

T30, T31, T32 = 2 ** 30, 2 ** 31, 2 ** 32
SMALL = 1 << 20          # operands below this many elements (weights, per-channel vectors, tables) are named in `small`, not listed as rows
SKIP = {"profile", "set_gemm_mode", "fused_modes", "gemm_mode", "set_halo", "set_rows_gemm", "rows_gemm", "empty_rows_bf16", "empty_rows",
        "empty_like_rows", "lane", "set_lane", "set_capture_key", "persistent_zeros", "drop_persistent", "persistent_bytes", "rows_view",
        "rows_gemm_ok", "cab_fused_ok", "aa_tables", "d4_check_codes", "d4_inverse_code", "d4_canonical_code"}


def operand(role, t):
    """(role, dtype, ld, channels, rows, extent) of a tensor whose last dim is contiguous; extent in elements."""
    if t.dim() < 2 or (t.stride(-1) != 1 and t.shape[-1] != 1):
        return dict(role=role, dtype=str(t.dtype).replace("torch.", ""), ld=int(t.shape[-1]) if t.dim() else 1, channels=int(t.shape[-1]) if t.dim() else 1,
                    rows=int(t.numel() // max(1, t.shape[-1] if t.dim() else 1)), extent=int(t.numel()))
    ld = int(t.stride(-2))
    rows = int(t.numel() // t.shape[-1])
    return dict(role=role, dtype=str(t.dtype).replace("torch.", ""), ld=ld, channels=int(t.shape[-1]), rows=rows, extent=rows * ld)


def conv2d_route(a):
    """ops.conv2d's choice, from its arguments (same order of tests)."""
    x, w, out = a["x"], a["w"], a.get("out")
    mode = ops.gemm_mode()
    (KH, KW), stride, pad = tuple(a["ksize"]), tuple(a["stride"]), tuple(a["pad"])
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    ldi, xp = x.stride(-2), x.data_ptr()
    op = out.data_ptr() if out is not None else -1
    c3 = (KH, KW) == (3, 3) and stride == (1, 1) and pad == (1, 1)
    if (mode != "f32" and c3 and Cout <= 16 and Cin * (1 if Cout == 1 else (4 if Cout <= 4 else 16)) <= 128 and a["shuffle"] == 0
            and a.get("mul") is None and not a["dynamic_w"] and H * W >= 4096 and xp != op):
        return "conv3x3_small", "small"
    if mode == "f32":
        return "igemm_f32", None
    halo_ok = (ops._HALO and c3 and not a["dynamic_w"] and Cin >= 32 and Cin % 4 == 0 and ldi % 4 == 0 and xp % 16 == 0
               and (Cout <= 64 or Cin >= 128 or 128 < Cout <= 192) and H * W >= 1024 and xp != op and B * H * W * ldi < T31)
    if halo_ok:
        return "halo", ("halo" if mode == "bf16x3" else "halo1")
    return "igemm_bf16s", "split"


def route_of(name, a):
    mode = ops.gemm_mode()
    if name == "conv2d":
        return conv2d_route(a)
    if name == "linear":
        if mode == "f32":
            return "igemm_f32", None
        if a["x"].dtype == torch.bfloat16 or a["rows_gemm"]:
            return "rows_gemm", "split"
        return "igemm_bf16s", "split"
    if name == "resize":
        x, out = a["x"], a.get("out")
        v4 = (a["mode"] == "bilinear" and a["layout"] == "nhwc" and x.shape[-1] % 4 == 0 and x.stride(-2) % 4 == 0 and x.data_ptr() % 16 == 0
              and (out is None or (out.stride(-2) % 4 == 0 and out.data_ptr() % 16 == 0)))
        return ("vec4" if v4 else "scalar") + "_" + a["mode"], None
    return name, None


def scalars(a):
    """The arguments that select a kernel form: numbers, strings, tuples; a tensor argument appears as an operand instead."""
    s = {}
    for k, v in a.items():
        if isinstance(v, (bool, int, str)) or v is None:
            if v not in (None, False, 0, "none") and k not in ("tile_hint",):
                s[k] = v
        elif isinstance(v, float):
            if k in ("alpha", "mul", "ka", "kb") and v != 1.0:
                s[k] = "!=1"
        elif isinstance(v, (tuple, list)) and all(isinstance(u, (int, float)) for u in v):
            s[k] = list(v)
        elif isinstance(v, dict):
            s[k] = {kk: vv for kk, vv in v.items() if isinstance(vv, (int, str))}
    return s


class Recorder:
    def __init__(self):
        self.rows = {}
        self.counts = {}

    def wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapped(*args, **kwargs):
            ba = sig.bind(*args, **kwargs)
            ba.apply_defaults()
            a = dict(ba.arguments)
            pre = {k: v for k, v in a.items() if isinstance(v, torch.Tensor)}
            big_in = any(operand(k, v)["extent"] >= T30 for k, v in pre.items())
            ret = fn(*args, **kwargs)
            outs = ret if isinstance(ret, tuple) else (ret,)
            tens = dict(pre)
            ptrs = {v.data_ptr() for v in pre.values()}
            for i, r in enumerate(outs):
                if isinstance(r, ops.PoolPartials):
                    tens[f"ret{i}.part"] = r.part
                elif isinstance(r, torch.Tensor) and r.data_ptr() not in ptrs:
                    tens[f"ret{i}"] = r
            opsd = [operand(k, v) for k, v in tens.items()]
            if not (big_in or any(o["extent"] >= T30 for o in opsd)):
                return ret
            route, kind = route_of(name, a)
            if kind is not None and kind not in [k for k, _ in ops.PREPARED.of(a["w"])] and not a.get("dynamic_w"):
                raise RuntimeError(f"{name}: derived route {route} but the weight has no {kind!r} image: {ops.PREPARED.of(a['w'])}")
            mode = ops.gemm_mode()
            small = sorted(o["role"] for o in opsd if o["role"] not in ("w", "w_tap") and o["extent"] < SMALL)
            shapes = {o["role"]: [o["dtype"], o["ld"], o["channels"], o["rows"]] for o in opsd if o["extent"] >= SMALL}
            if "w" in a and isinstance(a["w"], torch.Tensor):
                shapes["w"] = ["float32"] + [int(v) for v in a["w"].shape]
            call = json.dumps(dict(op=name, route=route, mode=mode, args=scalars(a), small=small, operands=shapes), sort_keys=True)
            self.counts[call] = self.counts.get(call, 0) + 1
            for o in opsd:
                if o["extent"] < SMALL:
                    continue
                key = (call, o["role"], o["dtype"], o["ld"], o["channels"], o["rows"])
                self.rows[key] = dict(op=name, route=route, mode=mode, call=call, role=o["role"], dtype=o["dtype"], ld=o["ld"], channels=o["channels"],
                                      rows=o["rows"], extent=o["extent"], ge31=o["extent"] >= T31, ge32=o["extent"] >= T32)
            return ret
        wrapped.__wrapped__ = fn
        return wrapped


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "bigextent_calls.json")
    import bench
    from isr2_amd.model import FreqFusionHIP
    from isr2_amd.weights import synth_state_dict
    dev = torch.device("cuda:0")
    sd = synth_state_dict(1234)
    lr = (bench.make_tile(44, 2048)[0, :, :1356, :2040].permute(1, 2, 0).numpy() * 255.0).round().astype(np.uint8)
    lr_t = torch.from_numpy(lr.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0).to(dev)
    rec = Recorder()
    for name, fn in list(vars(ops).items()):
        if inspect.isfunction(fn) and fn.__module__ == ops.__name__ and not name.startswith("_") and name not in SKIP:
            setattr(ops, name, rec.wrap(name, fn))
    runs = {}
    for mode in ("bf16x3", "bf16", "f32"):
        ops.set_gemm_mode(mode)
        model = FreqFusionHIP(sd, dev)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = model(lr_t)
        torch.cuda.synchronize()
        runs[mode] = dict(seconds=round(time.perf_counter() - t0, 2), peak_bytes=int(torch.cuda.max_memory_allocated()), shape=list(out.shape))
        print(mode, runs[mode], len(rec.rows), "rows so far", flush=True)
        del out, model
        ops.drop_persistent()
        ops._PERSIST_EAGER.clear()
        ops.PREPARED.clear()
        torch.cuda.empty_cache()
    ops.set_gemm_mode("bf16x3")
    rows = sorted(rec.rows.values(), key=lambda r: (r["op"], r["route"], r["mode"], r["call"], r["role"], r["ld"], r["rows"]))
    calls = sorted(rec.counts.items())
    blob = dict(image=dict(lr=[1356, 2040], hr=[5424, 8160], seed=44), forwards=runs,
                launches={c: n for c, n in calls}, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(blob, f, indent=1, sort_keys=True)
    print(f"wrote {out_path}: {len(rows)} rows of {len(calls)} distinct launches", flush=True)


if __name__ == "__main__":
    main()
