"""The training kernels of csrc/train_ops.hip held, element by element, to the fp64 references of tests/golden/train_ref.py:

    |kernel - ref| <= C_op * 2^-24 * mag

over the case tables of that module (tests/test_train_ref_cpu.py runs the same tables against fp32 stand-ins and their mutants on the
CPU).  The kernels are driven through the C ABI directly -- the only way to reach strides, accumulate and the workspaces -- and, where
a data or bias gradient belongs to the operation, through the tape as well.  Every direct call
  * gets exactly ff_*_workspace(...) floats inside a larger NaN-filled allocation, whose tail must still be NaN afterwards;
  * writes into NaN for accumulate = 0 and into a seeded tensor (part of ref and mag) for accumulate = 1;
  * sees NaN in the channels a row stride leaves unaddressed, and must leave the unaddressed channels of its output NaN.
Each test prints the worst ratio |d| / (2^-24 mag) it saw per kernel (TRAIN_KERNEL_RATIO lines); DESIGN.md quotes them next to the
CPU-measured constants.  Dropout stays on the finite-difference test of tests/test_train_ops_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 64
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _mode():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import ops
    old = ops.gemm_mode()
    ops.set_gemm_mode("f32")
    yield
    ops.set_gemm_mode(old)
    for k in sorted(WORST):
        print(f"TRAIN_KERNEL_RATIO {k}: {WORST[k]:.3f}")


def env():
    from isr2_amd import autograd as ag, lib as L
    return L.load(), L, ag._st()


def note(kernel, r):
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    return r


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def rows_buf(a, ld):
    """[rows, C] -> a device allocation [rows, ld] with a in the first C channels and NaN in the rest."""
    a = np.asarray(a, dtype=np.float32)
    rows, C = a.shape
    buf = np.full((rows, ld), NAN, np.float32)
    buf[:, :C] = a
    return dev(buf)


def out_buf(rows, C, ld, init=None):
    buf = np.full((rows, ld), NAN, np.float32)
    if init is not None:
        buf[:, :C] = np.asarray(init, dtype=np.float32).reshape(rows, C)
    return dev(buf)


def take(buf, C):
    """The addressed channels of an output allocation; the unaddressed ones must still be NaN."""
    h = host(buf)
    assert np.isnan(h[:, C:]).all(), "the kernel wrote channels beyond C"
    return h[:, :C]


def workspace(nw):
    assert nw >= 0
    return torch.full((int(nw) + GUARD,), NAN, device="cuda", dtype=torch.float32)


def guard_ok(work, nw):
    assert torch.isnan(work[int(nw):]).all().item(), "the kernel wrote beyond its workspace"


def ptr(t):
    return None if t is None else t.data_ptr()


def run_tape(build, inputs, gy):
    from isr2_amd import autograd as ag
    vs = {k: ag.Var(dev(v), True) for k, v in inputs.items()}
    with ag.Tape() as tape:
        y = build(vs)
        y.grad, y.owned = dev(gy), True
        tape.backward()
    torch.cuda.synchronize()
    return y.data.cpu().numpy(), {k: v.grad.cpu().numpy() for k, v in vs.items()}


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv2d_wgrad(case):
    lib, L, st = env()
    B, H, W, Cin, Cout, KH, KW = case
    x, dz, dw0, _ = R.wgrad_inputs(case)
    M = B * H * W
    refs = {acc: R.conv_wgrad_ref(x, dz, KH, KW, dw0 if acc else None) for acc in (0, 1)}
    nw = lib.ff_conv2d_wgrad_workspace(B, H, W, Cin, Cout, KH, KW)
    for ldx, ldz in ((Cin, Cout), (Cin + 7, Cout + 3)):
        xb, zb = rows_buf(x.reshape(M, Cin), ldx), rows_buf(dz.reshape(M, Cout), ldz)
        for acc in (0, 1):
            work = workspace(nw)
            dw = dev(dw0) if acc else torch.full((Cout, KH * KW * Cin), NAN, device="cuda")
            L.check(lib.ff_conv2d_wgrad(xb.data_ptr(), ldx, zb.data_ptr(), ldz, dw.data_ptr(), B, H, W, Cin, Cout, KH, KW, KH // 2, KW // 2, acc,
                                        work.data_ptr(), nw, st))
            got = host(dw)
            guard_ok(work, nw)
            note("conv2d_wgrad", R.check(got, *refs[acc], R.C_WGRAD, f"ff_conv2d_wgrad {case} ld=({ldx},{ldz}) acc={acc}"))
    print(f"conv2d_wgrad {case}: worst so far {WORST['conv2d_wgrad']:.2f} of {R.C_WGRAD:g}")


@pytest.mark.parametrize("case", R.WGRAD_SPATIAL, ids=lambda c: "x".join(map(str, c)))
def test_conv2d_tape_gradients(case):
    """dx (a forward convolution with the flipped weights), db (ff_reduce_cols) and dw through the tape."""
    from isr2_amd import autograd as ag
    B, H, W, Cin, Cout, KH, KW = case
    x, dz, _, w = R.wgrad_inputs(case)
    b = R.draw(9, Cout, scale=0.1)
    _, g = run_tape(lambda v: ag.conv2d(v["x"], v["w"], v["b"], ksize=(KH, KW)), dict(x=x, w=w, b=b), dz)
    r = [note("tape conv2d dx", R.check(g["x"], *R.conv_dgrad_ref(dz, w, KH, KW), R.C_WGRAD, f"dx {case}")),
         note("tape conv2d db", R.check(g["b"], *R.bias_grad_ref(dz), R.C_REDUCE, f"db {case}")),
         note("tape conv2d dw", R.check(g["w"], *R.conv_wgrad_ref(x, dz, KH, KW), R.C_WGRAD, f"dw {case}"))]
    print(f"tape conv2d {case}: dx {r[0]:.2f} db {r[1]:.2f} dw {r[2]:.2f}")


@pytest.mark.parametrize("k", R.DW_KERNELS, ids=lambda k: f"{k[0]}x{k[1]}")
@pytest.mark.parametrize("case", R.DWGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dwconv2d_wgrad(case, k):
    lib, L, st = env()
    B, H, W, C = case
    KH, KW = k
    x, dy, dw0 = R.dwgrad_inputs(case, k)
    M = B * H * W
    nw = lib.ff_dwconv2d_wgrad_workspace(B, H, W, C, KH, KW)
    for ldx, ldy in ((C, C), (C + 5, C + 2)):
        xb, yb = rows_buf(x.reshape(M, C), ldx), rows_buf(dy.reshape(M, C), ldy)
        for acc in (0, 1):
            work = workspace(nw)
            dw = dev(dw0) if acc else torch.full((KH * KW, C), NAN, device="cuda")
            L.check(lib.ff_dwconv2d_wgrad(xb.data_ptr(), ldx, yb.data_ptr(), ldy, dw.data_ptr(), B, H, W, C, KH, KW, acc, work.data_ptr(), nw, st))
            got = host(dw)
            guard_ok(work, nw)
            note("dwconv2d_wgrad", R.check(got, *R.dwconv_wgrad_ref(x, dy, KH, KW, dw0 if acc else None), R.C_DWGRAD,
                                           f"ff_dwconv2d_wgrad {case} {k} ld=({ldx},{ldy}) acc={acc}"))
    print(f"dwconv2d_wgrad {case} {k}: worst so far {WORST['dwconv2d_wgrad']:.2f} of {R.C_DWGRAD:g}")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.REDUCE_COLS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_reduce_cols(case):
    lib, L, st = env()
    rows, C, rpg = case
    G = rows // (rpg or rows)
    nw = lib.ff_reduce_cols_workspace(rows, C, rpg)
    out0 = R.draw(5, G, C)
    for y_kind in R.REDUCE_COLS_YKINDS:
        x, y = R.reduce_inputs(rows, C, y_kind)
        for ldx, ldy in ((C, {0: C, 1: 1, 4: 0}[y_kind]), (C + 3, {0: C + 6, 1: 4, 4: 0}[y_kind])):
            xb = rows_buf(x, ldx)
            yb = rows_buf(y, ldy) if y is not None else None
            for acc in (0, 1):
                work = workspace(nw)
                out = dev(out0) if acc else torch.full((G, C), NAN, device="cuda")
                L.check(lib.ff_reduce_cols(xb.data_ptr(), ldx, ptr(yb), ldy, y_kind, rows, C, rpg, R.REDUCE_SCALE, out.data_ptr(), acc,
                                           work.data_ptr(), nw, st))
                got = host(out)
                guard_ok(work, nw)
                note("reduce_cols", R.check(got, *R.reduce_cols_ref(x, y, rpg, R.REDUCE_SCALE, out0 if acc else None), R.C_REDUCE,
                                            f"ff_reduce_cols {case} y{y_kind} ld=({ldx},{ldy}) acc={acc}"))
    print(f"reduce_cols {case}: worst so far {WORST['reduce_cols']:.2f} of {R.C_REDUCE:g}")


@pytest.mark.parametrize("case", R.REDUCE_ROWS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_reduce_rows(case):
    lib, L, st = env()
    rows, C = case
    out0 = R.draw(5, rows)
    for y_kind in R.REDUCE_ROWS_YKINDS:
        x, y = R.reduce_inputs(rows, C, y_kind)
        for ldx, ldy, ldo in ((C, C, 1), (C + 3, C + 6, 5)):
            xb = rows_buf(x, ldx)
            yb = None if y is None else (rows_buf(y, ldy) if y_kind == 0 else dev(y))
            for acc in (0, 1):
                out = out_buf(rows, 1, ldo, out0 if acc else None)
                L.check(lib.ff_reduce_rows(xb.data_ptr(), ldx, ptr(yb), ldy if y_kind == 0 else 0, y_kind, rows, C, R.REDUCE_SCALE, out.data_ptr(),
                                           ldo, acc, st))
                note("reduce_rows", R.check(take(out, 1)[:, 0], *R.reduce_rows_ref(x, y, R.REDUCE_SCALE, out0 if acc else None), R.C_REDUCE,
                                            f"ff_reduce_rows {case} y{y_kind} ld=({ldx},{ldy},{ldo}) acc={acc}"))
    print(f"reduce_rows {case}: worst so far {WORST['reduce_rows']:.2f} of {R.C_REDUCE:g}")


@pytest.mark.parametrize("C", R.EW_FMA_CS)
def test_ew_fma(C):
    lib, L, st = env()
    rows, rpg = R.EW_FMA_ROWS, R.EW_FMA_RPG
    a = R.draw(1, rows, C)
    for strided in (False, True):
        lda, ldb, ldc, ldo = (C + 1, C + 2, C + 3, C + 4) if strided else (C, C, C, C)
        ab = rows_buf(a, lda)
        for bk, ck in R.EW_FMA_KINDS:
            b, c = R.fma_operand(bk, rows, C, rpg, 2), R.fma_operand(ck, rows, C, rpg, 3)
            put = lambda t, k, ld: None if t is None else (rows_buf(t, ld if k == 0 else (3 if strided else 1)) if k in (0, 1) else dev(t))
            bb, cb = put(b, bk, ldb), put(c, ck, ldc)
            ldbb = {0: ldb, 1: 3 if strided else 1}.get(bk, 0)
            ldcc = {0: ldc, 1: 3 if strided else 1}.get(ck, 0)
            for with_a in (True, False):
                for clamp in (0, 1):
                    out = out_buf(rows, C, ldo)
                    L.check(lib.ff_ew_fma(out.data_ptr(), ldo, ab.data_ptr() if with_a else None, lda, ptr(bb), ldbb, bk, ptr(cb), ldcc, ck,
                                          R.EW_FMA_SCALE, rows, C, rpg, clamp, st))
                    ref, mag = R.ew_fma_ref(a if with_a else None, b, bk, c, ck, R.EW_FMA_SCALE, rows, C, rpg, clamp)
                    note("ew_fma", R.check(take(out, C), ref, mag, R.C_EW_FMA, f"ff_ew_fma C={C} b{bk} c{ck} a={with_a} clamp={clamp} strided={strided}"))
    print(f"ew_fma C={C}: worst so far {WORST['ew_fma']:.2f} of {R.C_EW_FMA:g}")


@pytest.mark.parametrize("name", list(R.UNARY))
def test_ew_unary(name):
    lib, L, st = env()
    op, count, has_g = R.UNARY[name]
    x, g = R.unary_vector()
    ref, mag = R.unary_ref(name, x, g if has_g else None)
    C = 7                                                          # the vector as [rows, 7] rows: 4129 = 7 * 589 + 6 -> pad with 1.0
    n = -(-x.size // C) * C
    pad = lambda v: np.concatenate([v, np.ones(n - v.size, np.float32)]).reshape(-1, C)
    for ldx, ldg, ldo in ((C, C, C), (C + 2, C + 5, C + 1)):
        xb, gb = rows_buf(pad(x), ldx), rows_buf(pad(g), ldg)
        out = out_buf(n // C, C, ldo)
        L.check(lib.ff_ew_unary(op, xb.data_ptr(), ldx, gb.data_ptr() if has_g else None, ldg, out.data_ptr(), ldo, n // C, C, R.UNARY_P0, st))
        got = take(out, C).reshape(-1)[:x.size]
        note(f"ew_unary {name}", R.unary_check(name, got, ref, mag, f"ff_ew_unary {name} ld=({ldx},{ldg},{ldo})"))
    print(f"ew_unary {name}: worst {WORST[f'ew_unary {name}']:.2f} of {count}")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LN_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]:g}-{c[3]:g}")
def test_layernorm_bwd(case):
    lib, L, st = env()
    rows, C, eps, shift = case
    x, dy, gamma = R.ln_inputs(case)
    dgb0 = R.draw(9, 2, C)
    nw = lib.ff_layernorm_bwd_workspace(rows, C)
    gd = dev(gamma)
    refs = {acc: R.layernorm_bwd_ref(x, dy, gamma, eps, dgb0 if acc else None) for acc in (0, 1)}
    for ldx, ldy, lddx in ((C, C, C), (C + 3, C + 1, C + 2)) if rows <= 700 else ((C, C, C),):
        xb, yb = rows_buf(x, ldx), rows_buf(dy, ldy)
        for acc in (0, 1):
            work = workspace(nw)
            dx = out_buf(rows, C, lddx)
            dgb = dev(dgb0) if acc else torch.full((2, C), NAN, device="cuda")
            L.check(lib.ff_layernorm_bwd(xb.data_ptr(), ldx, yb.data_ptr(), ldy, gd.data_ptr(), eps, dx.data_ptr(), lddx, rows, C, dgb.data_ptr(), acc,
                                         work.data_ptr(), nw, st))
            gdx, gdgb = take(dx, C), host(dgb)
            guard_ok(work, nw)
            rdx, mdx, rgb, mgb = refs[acc]
            note("layernorm_bwd dx", R.check(gdx, rdx, mdx, R.C_LN_BWD, f"ff_layernorm_bwd dx {case} ld=({ldx},{ldy},{lddx}) acc={acc}"))
            note("layernorm_bwd dgamma|dbeta", R.check(gdgb, rgb, mgb, R.C_LN_BWD, f"ff_layernorm_bwd dgamma|dbeta {case} acc={acc}"))
    print(f"layernorm_bwd {case}: dx {WORST['layernorm_bwd dx']:.2f}, dgamma|dbeta {WORST['layernorm_bwd dgamma|dbeta']:.2f} of {R.C_LN_BWD:g} so far")


@pytest.mark.parametrize("hw", R.AVGPOOL_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_avgpool2_adj(hw):
    lib, L, st = env()
    H, W = hw
    B = 2
    for C in (1, 5):
        dy, dx0 = R.draw(1, B, H // 2, W // 2, C), R.draw(2, B, H, W, C)
        for ldy, ldx in ((C, C), (C + 3, C + 2)):
            yb = rows_buf(dy.reshape(-1, C), ldy)
            for acc in (0, 1):
                dx = out_buf(B * H * W, C, ldx, dx0 if acc else None)
                L.check(lib.ff_avgpool2_adj(yb.data_ptr(), ldy, dx.data_ptr(), ldx, B, H, W, C, acc, st))
                ref, mag = R.avgpool2_adj_ref(dy, H, W, dx0 if acc else None)
                note("avgpool2_adj", R.check(take(dx, C).reshape(B, H, W, C), ref, mag, R.C_AVGPOOL_ADJ, f"ff_avgpool2_adj {hw} C={C} acc={acc}"))
    print(f"avgpool2_adj {hw}: worst so far {WORST['avgpool2_adj']:.2f} of {R.C_AVGPOOL_ADJ:g}")


@pytest.mark.parametrize("hw", R.SPEC_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_spec_mask(hw):
    lib, L, st = env()
    H, W = hw
    Wf = W // 2 + 1
    for planes in R.SPEC_PLANES:
        X, gY, m, _, _ = R.spec_inputs(H, W, planes)
        Xd, gd, md = dev(X), dev(gY), dev(m)
        Y = torch.full((planes, H, Wf, 2), NAN, device="cuda")
        L.check(lib.ff_spec_mask_mul(Xd.data_ptr(), md.data_ptr(), Y.data_ptr(), planes, H, Wf, st))
        note("spec_mask_mul", R.check(host(Y), *R.spec_mask_mul_ref(X, m), R.C_SPEC_MUL, f"ff_spec_mask_mul {hw} x{planes}"))
        dm0 = R.draw(4, H, Wf)
        for acc in (0, 1):
            dm = dev(dm0) if acc else torch.full((H, Wf), NAN, device="cuda")
            L.check(lib.ff_spec_mask_grad(gd.data_ptr(), Xd.data_ptr(), dm.data_ptr(), planes, H, W, acc, st))
            note("spec_mask_grad", R.check(host(dm), *R.spec_mask_grad_ref(gY, X, W, dm0 if acc else None), R.C_REDUCE,
                                           f"ff_spec_mask_grad {hw} x{planes} acc={acc}"))
    print(f"spec_mask {hw}: mul {WORST['spec_mask_mul']:.2f} of {R.C_SPEC_MUL:g}, grad {WORST['spec_mask_grad']:.2f} of {R.C_REDUCE:g} so far")


@pytest.mark.parametrize("hw", R.SPEC_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_rfft2_irfft2(hw):
    from isr2_amd import autograd as ag
    lib, L, st = env()
    H, W = hw
    Wf = W // 2 + 1
    fft = ag.FFT2(torch.device("cuda:0"))
    (wc, ws), (hc, hs) = fft.tw(W), fft.tw(H)
    for planes in R.SPEC_PLANES:
        nw = planes * H * Wf * 2
        x = R.draw(21, planes, H, W)
        xd, work = dev(x), workspace(nw)
        spec = torch.full((planes, H, Wf, 2), NAN, device="cuda")
        L.check(lib.ff_rfft2(xd.data_ptr(), planes, H, W, wc.data_ptr(), ws.data_ptr(), hc.data_ptr(), hs.data_ptr(), work.data_ptr(), nw, spec.data_ptr(), st))
        got = host(spec)
        guard_ok(work, nw)
        note("rfft2", R.check(got, *R.rfft2_ref(x), R.C_DFT, f"ff_rfft2 {hw} x{planes}"))
        sp = R.spec_inputs(H, W, planes)[0] * R.draw(22, H, Wf)[None, :, :, None]
        sd, work = dev(sp), workspace(nw)
        out = torch.full((planes, H, W), NAN, device="cuda")
        L.check(lib.ff_irfft2(sd.data_ptr(), planes, H, W, wc.data_ptr(), ws.data_ptr(), hc.data_ptr(), hs.data_ptr(), work.data_ptr(), nw, out.data_ptr(), st))
        got = host(out)
        guard_ok(work, nw)
        note("irfft2", R.check(got, *R.irfft2_ref(sp, W), R.C_DFT, f"ff_irfft2 {hw} x{planes}"))
    print(f"rfft2 / irfft2 {hw}: {WORST['rfft2']:.2f}, {WORST['irfft2']:.2f} of {R.C_DFT:g} so far")


@pytest.mark.parametrize("case", R.MHA_CASES, ids=lambda c: f"nt{c[0]}-h{c[1]}-P{c[2]}-s{c[3]:g}")
def test_band_mha(case):
    lib, L, st = env()
    nt, heads, P, _ = case
    E = heads * 16
    qkv, dout = R.mha_inputs(case)
    out, outm, dqkv, dqkvm = R.band_mha_ref(qkv, dout, P, nt, heads)
    qd, gd = dev(qkv), dev(dout)
    o = torch.full((P * nt, E), NAN, device="cuda")
    L.check(lib.ff_band_mha_train(qd.data_ptr(), o.data_ptr(), P, nt, heads, 0.0, 0, st))
    nw = lib.ff_band_mha_bwd_workspace(P, nt, heads)
    work = workspace(nw)
    dq = torch.full((P * nt, 3 * E), NAN, device="cuda")
    L.check(lib.ff_band_mha_bwd(qd.data_ptr(), gd.data_ptr(), dq.data_ptr(), P, nt, heads, 0.0, 0, work.data_ptr(), nw, st))
    go, gq = host(o), host(dq)
    guard_ok(work, nw)
    r = (note("band_mha_train", R.check(go, out, outm, R.C_MHA_BWD, f"ff_band_mha_train {case}")),
         note("band_mha_bwd", R.check(gq, dqkv, dqkvm, R.C_MHA_BWD, f"ff_band_mha_bwd {case}")))
    print(f"band_mha {case}: out {r[0]:.2f}, dqkv {r[1]:.2f} of {R.C_MHA_BWD:g}")


@pytest.mark.parametrize("case", R.BN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_batchnorm_train(case):
    """Through the tape (column sums, ff_bn_train_finish, ff_bn_xhat, ff_bn_train_bwd, running statistics), then ff_bn_xhat and
    ff_bn_train_bwd directly with row strides, fed the reference's statistics rounded to fp32."""
    from isr2_amd import autograd as ag
    lib, L, st = env()
    G, C, rpg = case
    rows = G * rpg
    i = R.bn_inputs(case)
    ref = R.batchnorm_train_ref(i["x"], i["gamma"], i["beta"], i["rm0"], i["rv0"], i["dy"], G)
    rmd, rvd = dev(i["rm0"]), dev(i["rv0"])
    y, g = run_tape(lambda v: ag.batchnorm_train(v["x"], v["gamma"], v["beta"], rmd, rvd, groups=G, eps=R.BN_EPS, momentum=R.BN_MOMENTUM),
                    dict(x=i["x"], gamma=i["gamma"], beta=i["beta"]), i["dy"])
    got = dict(y=y, dx=g["x"], dgamma=g["gamma"], dbeta=g["beta"], running_mean=host(rmd), running_var=host(rvd))
    for k, v in got.items():
        note(f"batchnorm_train {k}", R.check(v, *ref[k], getattr(R, R.BN_CONST[k]), f"tape batchnorm_train {k} {case}"))
    mr, sdy, sdyxh, gd = dev(ref["mean_rstd"]), dev(ref["sdy"]), dev(ref["sdyxh"]), dev(i["gamma"])
    ldx, ldy, lddx, ldh = C + 3, C + 1, C + 2, C + 4
    xb, yb, dx, xh = rows_buf(i["x"], ldx), rows_buf(i["dy"], ldy), out_buf(rows, C, lddx), out_buf(rows, C, ldh)
    L.check(lib.ff_bn_xhat(xb.data_ptr(), ldx, mr.data_ptr(), xh.data_ptr(), ldh, rows, C, rpg, st))
    L.check(lib.ff_bn_train_bwd(xb.data_ptr(), ldx, yb.data_ptr(), ldy, mr.data_ptr(), gd.data_ptr(), sdy.data_ptr(), sdyxh.data_ptr(), dx.data_ptr(),
                                lddx, rows, C, rpg, st))
    note("bn_xhat", R.check(take(xh, C), *ref["xhat"], R.C_BN_BWD, f"ff_bn_xhat {case}"))
    note("bn_train_bwd", R.check(take(dx, C), *ref["dx"], R.C_BN_BWD, f"ff_bn_train_bwd {case}"))
    print(f"batchnorm_train {case}: " + ", ".join(f"{k.split()[-1]} {v:.2f}" for k, v in sorted(WORST.items()) if k.startswith("batchnorm") or k.startswith("bn_")))


@pytest.mark.parametrize("case", R.BN_FINISH_CASES, ids=lambda c: "-".join(f"{v:g}" for v in c))
def test_bn_train_finish(case):
    """ff_bn_train_finish from given column sums, both forms of the variance (the tape only uses the centred one)."""
    lib, L, st = env()
    G, C, n, _, _ = case
    for centered in (0, 1):
        i = R.bn_finish_inputs(case, centered)
        ref = R.bn_finish_ref(i["s1"], i["s2"], centered, n, i["gamma"], i["beta"], i["rm0"], i["rv0"])
        d = {k: dev(v) for k, v in i.items()}
        mr, sc, sh = (torch.full(shape, NAN, device="cuda") for shape in ((G, C, 2), (G, C), (G, C)))
        L.check(lib.ff_bn_train_finish(d["s1"].data_ptr(), d["s2"].data_ptr(), centered, G, C, n, d["gamma"].data_ptr(), d["beta"].data_ptr(), R.BN_EPS,
                                       R.BN_MOMENTUM, d["rm0"].data_ptr(), d["rv0"].data_ptr(), mr.data_ptr(), sc.data_ptr(), sh.data_ptr(), st))
        for k, t in (("mean_rstd", mr), ("scale", sc), ("shift", sh), ("running_mean", d["rm0"]), ("running_var", d["rv0"])):
            note(f"bn_train_finish {k}", R.check(host(t), *ref[k], R.C_BN_FINISH, f"ff_bn_train_finish {k} {case} centered={centered}"))
    print(f"bn_train_finish {case}: " + ", ".join(f"{k.split()[-1]} {v:.2f}" for k, v in sorted(WORST.items()) if k.startswith("bn_train_finish")) + f" of {R.C_BN_FINISH:g}")


@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_resize_bilinear_adj(case):
    lib, L, st = env()
    Hi, Wi, Ho, Wo, sf = case
    B = 2
    sh, sw = R.aten_scale(Hi, Ho, sf), R.aten_scale(Wi, Wo, sf)
    for C in (1, 5):
        dy, dx0 = R.draw(1, B, Ho, Wo, C), R.draw(2, B, Hi, Wi, C)
        for ldy, ldx in ((C, C), (C + 3, C + 2)):
            yb = rows_buf(dy.reshape(-1, C), ldy)
            for acc in (0, 1):
                dx = out_buf(B * Hi * Wi, C, ldx, dx0 if acc else None)
                L.check(lib.ff_resize_bilinear_adj(yb.data_ptr(), ldy, Ho, Wo, dx.data_ptr(), ldx, Hi, Wi, B, C, sh, sw, R.RESIZE_MUL, acc, st))
                ref, mag = R.resize_adj_ref(dy, Hi, Wi, sh, sw, R.RESIZE_MUL, dx0 if acc else None)
                note("resize_bilinear_adj", R.check(take(dx, C).reshape(B, Hi, Wi, C), ref, mag, R.C_RESIZE_ADJ, f"ff_resize_bilinear_adj {case} C={C} acc={acc}"))
    print(f"resize_bilinear_adj {case}: worst so far {WORST['resize_bilinear_adj']:.2f} of {R.C_RESIZE_ADJ:g}")


@pytest.mark.parametrize("n", R.FLAT_NS)
def test_adamw_ema_step(n):
    lib, L, st = env()
    i = R.adamw_inputs(n)
    sq = np.float32((R.f64(i["g"]) ** 2).sum())
    for max_norm in (1e3, 0.5 * float(np.sqrt(sq)), 0.0):                     # clip inactive, active, off
        hyper = R.adamw_hyper(max_norm)
        hd, sd = dev(hyper), dev(np.array([sq]))
        for with_ema in (True, False):
            d = {k: dev(v) for k, v in i.items()}
            L.check(lib.ff_adamw_ema_step(d["p"].data_ptr(), d["g"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(),
                                          d["ema"].data_ptr() if with_ema else None, n, hd.data_ptr(), sd.data_ptr(), st))
            ref = R.adamw_ema_ref(i["p"], i["g"], i["m"], i["v"], i["ema"] if with_ema else None, hyper, sq)
            for k in ref:
                note(f"adamw_ema_step {k}", R.check(host(d[k]), *ref[k], R.C_ADAMW, f"ff_adamw_ema_step {k} n={n} max_norm={max_norm:g}", floor=R.FLT_MIN))
            if not with_ema:
                assert np.array_equal(host(d["ema"]), i["ema"]), "ema written although the pointer was null"
    print(f"adamw_ema_step n={n}: " + ", ".join(f"{k.split()[-1]} {v:.2f}" for k, v in sorted(WORST.items()) if k.startswith("adamw")) + f" of {R.C_ADAMW:g}")


@pytest.mark.parametrize("n", R.FLAT_NS)
def test_l1_loss_grad_and_sqnorm(n):
    lib, L, st = env()
    sr, hr = R.l1_inputs(n)
    loss_ref, loss_mag, dsr_ref = R.l1_loss_grad_ref(sr, hr)
    work = workspace(1024)
    dsr, loss = torch.full((n,), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    srd, hrd = dev(sr), dev(hr)
    L.check(lib.ff_l1_loss_grad(srd.data_ptr(), hrd.data_ptr(), dsr.data_ptr(), n, loss.data_ptr(), work.data_ptr(), 1024, st))
    gl, gd = host(loss), host(dsr)
    guard_ok(work, 1024)
    r0 = note("l1_loss", R.check(gl, loss_ref, loss_mag, R.c_flat_sum(n), f"ff_l1_loss_grad loss n={n}"))
    assert np.array_equal(gd.astype(np.float64), dsr_ref), "ff_l1_loss_grad: dsr is +-fp32(1/n) inside [0, 1] (bounds included), 0 where sr = hr or outside"
    g = R.draw(7, n, scale=0.01)
    work = workspace(1024)
    sq = torch.full((1,), NAN, device="cuda")
    gdev = dev(g)
    L.check(lib.ff_grad_sqnorm(gdev.data_ptr(), n, sq.data_ptr(), work.data_ptr(), 1024, st))
    gs = host(sq)
    guard_ok(work, 1024)
    r1 = note("grad_sqnorm", R.check(gs, *R.sqnorm_ref(g), R.c_flat_sum(n), f"ff_grad_sqnorm n={n}"))
    print(f"l1 / sqnorm n={n}: {r0:.2f}, {r1:.2f} of {R.c_flat_sum(n)}")


def test_exact_data_movement():
    lib, L, st = env()
    for A, Bd, C in R.PERMUTE_CASES:
        x = R.draw(1, A * Bd, C)
        out = torch.full((Bd * A, C), NAN, device="cuda")
        xd = dev(x)
        L.check(lib.ff_permute_rows(xd.data_ptr(), out.data_ptr(), A, Bd, C, st))
        assert np.array_equal(host(out).reshape(Bd, A, C), R.permute_rows_ref(x, A, Bd, C)), ("ff_permute_rows", A, Bd, C)
    for taps, C in R.TAPS_CASES:
        w = R.draw(2, taps, C)
        out = torch.full((taps, C), NAN, device="cuda")
        wd = dev(w)
        L.check(lib.ff_taps_reverse(wd.data_ptr(), out.data_ptr(), taps, C, st))
        assert np.array_equal(host(out), R.taps_reverse_ref(w)), ("ff_taps_reverse", taps, C)
    for Cout, Cin, KH, KW in R.FLIPT_CASES:
        w = R.draw(3, Cout, KH * KW * Cin)
        out = torch.full((Cin, KH * KW * Cout), NAN, device="cuda")
        wd = dev(w)
        L.check(lib.ff_conv_weight_flipT(wd.data_ptr(), out.data_ptr(), Cout, Cin, KH, KW, st))
        assert np.array_equal(host(out).reshape(Cin, KH * KW, Cout), R.conv_weight_flipT_ref(w, Cout, Cin, KH * KW)), ("ff_conv_weight_flipT", Cout, Cin, KH, KW)
