"""DAT's channel attention held, element by element, to the fp64 references of tests/golden/chan_ref.py:

    |kernel - ref| <= C * 2^-24 * mag + extra

over the case tables of that module (tests/test_chan_ref_cpu.py runs the same tables against fp32 stand-ins and their mutants on the
CPU).  The entries are driven through the C ABI directly, so that `work` is visible: what is compared first is every per-workgroup
partial block ff_chan_qkv and chan_gram_kernel leave there, then G and the 180 x 180 matrix after the entry's own finish.  Every call
  * gets the floats the entry claims inside a larger NaN-filled allocation: the partial blocks must come back finite, whatever lies
    beyond the claim must still be NaN;
  * sees NaN in the columns a row stride leaves unaddressed, and must leave the unaddressed columns of v at their sentinel;
  * is repeated once and must return the same bits.
Each test records the worst err / bound it saw per kernel and family (CHAN_ATTN_RATIO lines); DESIGN.md and
profiles/chan_attn_parity.json quote them next to the CPU-measured constants."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import chan_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 4096
SENTINEL = 12345.0
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import ops
    old = ops.gemm_mode()
    yield
    ops.set_gemm_mode(old)
    for k in sorted(WORST):
        print(f"CHAN_ATTN_RATIO {k}: {WORST[k]:.4f}")


@pytest.fixture(autouse=True)
def _stop_on_device_error():
    """A device error ends the module's run: nothing more is launched on a GPU that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def env():
    from isr2_amd import lib as L, ops
    return L.load(), L, ops._stream()


def note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def dev(t):
    return torch.as_tensor(t).float().contiguous().cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu()


def workspace(claim):
    return torch.full((int(claim) + GUARD,), NAN, device="cuda", dtype=torch.float32)


def guard_ok(work, claim):
    assert torch.isnan(work[int(claim):]).all().item(), "the entry wrote beyond the workspace it claims"


def rows_buf(a, ld, fill):
    buf = torch.full((a.shape[0], ld), fill, dtype=torch.float32)
    buf[:, :a.shape[1]] = a
    return buf.cuda()


def check_finish(work, nblk, wbd, key, what, base=0, gbase=None):
    """G and wbd of one image against chan_finish_ref of the partial blocks the kernels READ (taken back from `work`)."""
    part = work[base:base + nblk * R.BLK].reshape(nblk, R.BLK)
    gbase = base + nblk * R.BLK if gbase is None else gbase
    ref = R.chan_finish_ref(part, R.TEMPERATURE)
    rg = note(f"{key} G", R.check(work[gbase:gbase + R.BLK].numpy(), ref["G"].numpy(), ref["G_mag"].numpy(), R.C_REDUCE, f"{what}: G"))
    rw = note(f"{key} wbd", R.check(wbd.numpy(), ref["wbd"].numpy(), ref["wbd_mag"].numpy(), R.C_WBD, f"{what}: wbd"))
    return rg, rw


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.QKV_CASES, ids=R.case_name)
def test_chan_qkv_blocks(case):
    lib, L, st = env()
    from isr2_amd.prep import pack_chan_qkv
    M, ld, fam, nterms = case["M"], case["ld"], case["family"], case["nterms"]
    name = R.case_name(case)
    inp, ref = R.qkv_reference(M, fam, nterms)
    if fam == "exact":
        R.assert_exact(ref["facts"], name)
    nblk = ref["nblk"]
    claim = (nblk + 1) * R.BLK
    assert lib.ff_chan_qkv_workspace(M) >= claim
    pk = pack_chan_qkv(inp["wqkv"].float(), inp["bqkv"].float())
    w, b, gamma, beta, temp = pk["w"].cuda(), pk["b"].cuda(), dev(inp["gamma"]), dev(inp["beta"]), dev(R.TEMPERATURE)
    xb = rows_buf(inp["x"], ld, NAN)
    runs = []
    for _ in range(2):
        vb = torch.full((M, ld), SENTINEL, device="cuda", dtype=torch.float32)
        work = workspace(claim)
        L.check(lib.ff_chan_qkv(xb.data_ptr(), ld, M, R.C, gamma.data_ptr(), beta.data_ptr(), float(inp["eps"]), w.data_ptr(), b.data_ptr(),
                                vb.data_ptr(), ld, work.data_ptr(), claim, nterms, st))
        h = host(work)
        assert torch.isfinite(h[:nblk * R.BLK]).all().item(), "a partial block holds a float the kernel did not write"
        assert torch.isnan(h[nblk * R.BLK:]).all().item(), "ff_chan_qkv wrote beyond its nblk partial blocks"
        wbd = torch.full((R.C, R.C), NAN, device="cuda", dtype=torch.float32)
        L.check(lib.ff_chan_attn_finish(work.data_ptr(), claim, nblk, temp.data_ptr(), wbd.data_ptr(), st))
        runs.append((host(work), host(vb), host(wbd)))
        guard_ok(runs[-1][0], claim)
    (h, v, wbd), (h2, v2, wbd2) = runs
    assert torch.equal(h[:claim], h2[:claim]) and torch.equal(v, v2) and torch.equal(wbd, wbd2), "a second call differs"
    assert bool((v[:, R.C:] == SENTINEL).all()), "v's unaddressed columns were written"
    key = f"chan_qkv<{nterms}> {fam}"
    r = note(f"{key} partials", R.check(h[:nblk * R.BLK].reshape(nblk, R.BLK).numpy(), ref["part"].numpy(), ref["part_mag"].numpy(), R.C_PART,
                                        f"ff_chan_qkv {name}: partial blocks", ref["part_extra"].numpy()))
    if fam == "exact":
        assert torch.equal(v[:, :R.C].double(), ref["v"]), f"ff_chan_qkv {name}: v is not bit-equal"
        rv = 0.0
    else:
        rv = note(f"{key} v", float(((v[:, :R.C].double() - ref["v"]).abs() / R.v_bound(ref)).max()))
        assert rv <= 1.0, f"ff_chan_qkv {name}: v err / bound = {rv:.3g}"
    rg, rw = check_finish(h, nblk, wbd, "finish after chan_qkv", f"ff_chan_attn_finish {name}")
    print(f"chan_qkv {name}: err / bound partials {r:.4f}, v {rv:.4f}, G {rg:.4f}, wbd {rw:.4f}")


@pytest.mark.parametrize("case", R.GRAM_CASES, ids=R.case_name)
def test_chan_attn_weights_blocks(case):
    lib, L, st = env()
    N, ld, q_off, k_off = case["N"], case["ld"], case["q_off"], case["k_off"]
    name = R.case_name(case)
    qkv, (ref, mag) = R.gram_reference(**case)
    nblk, _ = R.gram_plan(N)
    claim = int(lib.ff_chan_attn_workspace(N))
    assert claim >= (nblk + 1) * R.BLK
    qb, temp = qkv.cuda(), dev(R.TEMPERATURE)
    runs = []
    for _ in range(2):
        work = workspace(claim)
        wbd = torch.full((R.C, R.C), NAN, device="cuda", dtype=torch.float32)
        L.check(lib.ff_chan_attn_weights(qb.data_ptr(), ld, q_off, k_off, N, temp.data_ptr(), wbd.data_ptr(), work.data_ptr(), claim, st))
        runs.append((host(work), host(wbd)))
        guard_ok(runs[-1][0], claim)
    (h, wbd), (h2, wbd2) = runs
    assert torch.equal(h[:(nblk + 1) * R.BLK], h2[:(nblk + 1) * R.BLK]) and torch.equal(wbd, wbd2), "a second call differs"
    assert torch.isfinite(h[:(nblk + 1) * R.BLK]).all().item() and torch.isnan(h[(nblk + 1) * R.BLK:]).all().item()
    r = note("chan_gram partials", R.check(h[:nblk * R.BLK].reshape(nblk, R.BLK).numpy(), ref.numpy(), mag.numpy(), R.C_PART,
                                           f"chan_gram_kernel {name}: partial blocks"))
    rg, rw = check_finish(h, nblk, wbd, "finish after chan_gram", f"ff_chan_attn_weights {name}")
    print(f"chan_attn_weights {name}: err / bound partials {r:.4f}, G {rg:.4f}, wbd {rw:.4f}")


@pytest.mark.parametrize("nblk", R.FINISH_NBLK)
def test_chan_attn_finish_synthetic(nblk):
    lib, L, st = env()
    p, ref = R.finish_reference(nblk)
    claim = (nblk + 1) * R.BLK
    work = workspace(claim)
    work[:nblk * R.BLK] = p.reshape(-1).cuda()
    wbd = torch.full((R.C, R.C), NAN, device="cuda", dtype=torch.float32)
    L.check(lib.ff_chan_attn_finish(work.data_ptr(), claim, nblk, dev(R.TEMPERATURE).data_ptr(), wbd.data_ptr(), st))
    h, wbd = host(work), host(wbd)
    guard_ok(h, claim)
    assert torch.equal(h[:nblk * R.BLK], p.reshape(-1)), "the partials were changed"
    rg = note("finish synthetic G", R.check(h[nblk * R.BLK:claim].numpy(), ref["G"].numpy(), ref["G_mag"].numpy(), R.C_REDUCE, f"finish nblk={nblk}: G"))
    rw = note("finish synthetic wbd", R.check(wbd.numpy(), ref["wbd"].numpy(), ref["wbd_mag"].numpy(), R.C_WBD, f"finish nblk={nblk}: wbd"))
    row = wbd[R.ZERO_Q, R.ZERO_Q // R.D * R.D:(R.ZERO_Q // R.D + 1) * R.D]
    assert bool((row == row[0]).all()) and abs(row[0].item() - 1.0 / R.D) < 1e-7, "a zero-norm q channel must give a uniform row"
    print(f"chan_attn_finish nblk={nblk}: err / bound G {rg:.4f}, wbd {rw:.4f}")


@pytest.mark.parametrize("case", R.FINISH_IMAGES, ids=R.case_name)
def test_chan_attn_finish_images_synthetic(case):
    lib, L, st = env()
    B, nblk = case["B"], case["nblk"]
    imgs = [R.finish_reference(nblk, 4600 + 10 * i + nblk) for i in range(B)]
    claim = B * (nblk + 1) * R.BLK
    work = workspace(claim)
    work[:B * nblk * R.BLK] = torch.cat([p.reshape(-1) for p, _ in imgs]).cuda()
    wbd = torch.full((B, R.C, R.C), NAN, device="cuda", dtype=torch.float32)
    L.check(lib.ff_chan_attn_finish_images(work.data_ptr(), claim, B, nblk * 256, dev(R.TEMPERATURE).data_ptr(), wbd.data_ptr(), st))
    h, wbd = host(work), host(wbd)
    guard_ok(h, claim)
    for i, (p, ref) in enumerate(imgs):
        g0 = (B * nblk + i) * R.BLK
        note("finish_images G", R.check(h[g0:g0 + R.BLK].numpy(), ref["G"].numpy(), ref["G_mag"].numpy(), R.C_REDUCE, f"finish_images {case} image {i}: G"))
        note("finish_images wbd", R.check(wbd[i].numpy(), ref["wbd"].numpy(), ref["wbd_mag"].numpy(), R.C_WBD, f"finish_images {case} image {i}: wbd"))
    print(f"chan_attn_finish_images {case}: err / bound G {WORST['finish_images G']:.4f}, wbd {WORST['finish_images wbd']:.4f}")


# ---------------------------------------------------------------------------------------------------------------------
# end to end through isr2_amd.ops, against chan_finish_ref of the REFERENCE partials with the propagated bound
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_chan_qkv_attn_end_to_end(mode):
    from isr2_amd import ops
    from isr2_amd.prep import pack_chan_qkv
    nterms = 3 if mode == "bf16x3" else 1
    inp, ref = R.qkv_reference(3000, "corr", nterms)
    fin = R.chan_finish_ref(ref["part"], R.TEMPERATURE, R.part_bound(ref["part_mag"], ref["part_extra"]))
    ops.set_gemm_mode(mode)
    pk = pack_chan_qkv(dev(inp["wqkv"]), dev(inp["bqkv"]))
    v, wbd = ops.chan_qkv_attn(dev(inp["x"]), pk, dev(inp["gamma"]), dev(inp["beta"]), dev(R.TEMPERATURE), eps=inp["eps"])
    wbd, v = host(wbd), host(v)
    r = note(f"chan_qkv_attn {mode} wbd", R.check(wbd.numpy(), fin["wbd"].numpy(), fin["wbd_mag"].numpy(), R.C_WBD, f"ops.chan_qkv_attn {mode}: wbd",
                                                  fin["wbd_extra"].numpy()))
    rv = note(f"chan_qkv_attn {mode} v", float(((v.double() - ref["v"]).abs() / R.v_bound(ref)).max()))
    assert rv <= 1.0, rv
    plain = float((wbd.double() - fin["wbd"]).abs().max())
    print(f"chan_qkv_attn {mode}: wbd err / bound {r:.4f} (max |d| {plain:.2e}, largest weight {fin['wbd'].max().item():.2f}, logit spread "
          f"{fin['spread']:.1f}), v {rv:.4f}")


def test_chan_attn_weights_end_to_end():
    from isr2_amd import ops
    case = R.GRAM_CASES[3]
    qkv, (part, mag) = R.gram_reference(**case)
    fin = R.chan_finish_ref(part, R.TEMPERATURE, R.part_bound(mag))
    ops.set_gemm_mode("f32")
    wbd = host(ops.chan_attn_weights(qkv.cuda(), case["q_off"], case["k_off"], dev(R.TEMPERATURE)))
    r = note("chan_attn_weights f32 wbd", R.check(wbd.numpy(), fin["wbd"].numpy(), fin["wbd_mag"].numpy(), R.C_WBD, "ops.chan_attn_weights f32: wbd",
                                                  fin["wbd_extra"].numpy()))
    print(f"chan_attn_weights f32: wbd err / bound {r:.4f} (max |d| {float((wbd.double() - fin['wbd']).abs().max()):.2e}, logit spread {fin['spread']:.1f})")
