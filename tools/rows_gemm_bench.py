"""Per-shape A/B of NAFNet's deep 1x1 GEMMs in plain bf16: fp32 rows through ff_conv2d_bf16s (the old route) against bf16 rows through
ff_gemm_rows_bf16 (every tile form), alternating in ONE process on device tensors (tuning aid; not part of the product or the tests).

    python tools/rows_gemm_bench.py [out.json] [rounds] [launches per timing]

Per shape and variant: `rounds` timings of `launches` back-to-back launches each, the variants interleaved inside every round; the table
gives the median and the min..max spread in microseconds per launch.  Operands are random (never zeros)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from isr2_amd import lib, ops  # noqa: E402

LEVELS = [("mid", 4096, 1024), ("lvl3", 16384, 512), ("lvl2", 65536, 256)]      # name, M, K = c at the 256 x 256 bench tile
EPIS = [("c1", 2, "plain"), ("c3", 1, "kmul"), ("c4", 2, "gate"), ("c5", 1, "res")]     # name, N / c, epilogue (kmul: fp32 A rows, scaled)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    ops.set_gemm_mode("bf16")
    L = lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    table = []
    for lname, M, K in LEVELS:
        for ename, nf, epi in EPIS:
            N = nf * K
            gate = epi == "gate"
            No = N // 2 if gate else N
            a32 = torch.randn(M, K, device=dev)
            a16 = a32.to(torch.bfloat16)
            kmul = None
            if epi == "kmul":
                kmul = torch.rand(K, device=dev) + 0.5
            else:
                a32 = a16.float()
            w = torch.randn(N, K, device=dev) / K ** 0.5
            hi = ops._split_weight(w, True, K)[0]
            bias = torch.randn(N, device=dev)
            mul = torch.randn(N, device=dev) if epi in ("res", "kmul") else None
            res = torch.randn(M, N, device=dev) if epi in ("res", "kmul") else None
            o32 = torch.empty(M, No, device=dev)
            o16 = torch.empty(M, No, device=dev, dtype=torch.bfloat16)
            p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

            def old():
                lib.check(L.ff_conv2d_bf16s(a32.data_ptr(), hi.data_ptr(), None, K, K, p(bias), p(mul), p(res), o32.data_ptr(), 1, 1, M, K, K,
                                            1, M, N, No, N, 1, 1, 1, 1, 0, 0, 0, 1.0, 1 if gate else 0, 1, 0, p(kmul), st))

            def new(hint):
                def f():
                    lib.check(L.ff_gemm_rows_bf16((a32 if kmul is not None else a16).data_ptr(), 1 if kmul is not None else 0, K, hi.data_ptr(), K, p(kmul),
                                                  p(bias), p(mul), p(res), N, (o16 if gate else o32).data_ptr(),
                                                  No, M, N, K, 1 if gate else 0, hint, st))
                return f
            variants = [("old", old)] + [(f"new_t{h}", new(h)) for h in (0, 1, 2)]
            for _, f in variants:
                f()
            torch.cuda.synchronize()
            got = (o16 if gate else o32).clone()
            old()
            torch.cuda.synchronize()
            equal = bool(torch.equal(got, o32.to(torch.bfloat16) if gate else o32))
            times = {v: [] for v, _ in variants}
            for _ in range(rounds):
                for v, f in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    times[v].append(e0.elapsed_time(e1) * 1e3 / n)
            row = dict(level=lname, conv=ename, M=M, K=K, N=N, epilogue=epi, bit_equal=equal, gflop=2.0 * M * N * K / 1e9,
                       us={v: dict(median=round(statistics.median(t), 2), min=round(min(t), 2), max=round(max(t), 2)) for v, t in times.items()})
            table.append(row)
            print(f"{lname:5s} {ename} {M:6d} x {K:4d} -> {N:4d} equal={equal} " +
                  " | ".join(f"{v} {d['median']:7.1f} ({d['min']:.1f}..{d['max']:.1f})" for v, d in row["us"].items()), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        json.dump(dict(tool="tools/rows_gemm_bench.py", rounds=rounds, launches_per_timing=n, unit="us per launch", shapes=table),
                  open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
