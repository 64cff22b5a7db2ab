"""HAT OCAB on head-padded bf16 rows (plain bf16): ff_token_linear_rows16 writes q (scaled) / k / v as bf16 rows with every head slice
padded from 30 to 32 channels, ff_ocab_attn_rows16 reads them.  The contract is bit-equality with what they replace: the fp32 rows
of ff_token_linear(nterms = 1) rounded the way ff_ocab_attn rounds them on arrival (q after the scale), and ff_ocab_attn itself on
those fp32 rows.  torch.equal throughout; every launch is made once."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HEADS, D, K = 6, 30, 180
C = HEADS * D


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isr2_amd import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture
def bf16_mode(dev):
    from isr2_amd import ops
    old = ops.gemm_mode()
    ops.set_gemm_mode("bf16")
    yield ops
    ops.set_gemm_mode(old)


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def _perm(dev):
    """Column 32 t + j of the padded rows <- channel 180 (t // 6) + 30 (t % 6) + j of the fp32 rows; pad columns -> -1."""
    p = torch.full((576,), -1, dtype=torch.long)
    for t in range(18):
        p[32 * t:32 * t + D] = C * (t // HEADS) + D * (t % HEADS) + torch.arange(D)
    return p.to(dev)


@pytest.mark.parametrize("ln", [True, False])
def test_qkv_rows16_equals_rounded_token_linear(bf16_mode, dev, ln):
    ops = bf16_mode
    from isr2_amd.prep import pack_ocab_qkv, pack_token_linear
    M = 300                                                         # a ragged last 32-row tile (and a ragged second workgroup)
    w, b = rnd(3 * C, K, dev=dev, seed=1, scale=K ** -0.5), rnd(3 * C, dev=dev, seed=2)
    x = rnd(M, K, dev=dev, seed=3)
    g, be = (1.0 + 0.1 * rnd(K, dev=dev, seed=4), 0.1 * rnd(K, dev=dev, seed=5)) if ln else (None, None)
    want32 = ops.token_linear(x, pack_token_linear(w, b), gamma=g, beta=be)
    pk = pack_ocab_qkv(w, b, HEADS, D)
    SENT = -7.5                                                     # exactly representable in bf16
    buf = torch.full((M + 40, 640), SENT, device=dev, dtype=torch.bfloat16)
    got = ops.token_linear_rows16(x, pk, gamma=g, beta=be, out=buf[:M, :576])
    assert got.data_ptr() == buf.data_ptr()
    perm = _perm(dev)
    real = perm >= 0
    want = (want32[:, perm[real]] * pk["scale"][real]).bfloat16()
    assert torch.equal(buf[:M, :576][:, real], want)
    assert torch.count_nonzero(buf[:M, :576][:, ~real]) == 0
    assert int(real.sum()) == 540 and torch.count_nonzero(want) > 0.99 * want.numel()
    assert torch.all(buf[M:] == SENT) and torch.all(buf[:, 576:] == SENT)


def _padded_rows(qkv32, scale, dev):
    """The bf16 rows the rows form reads, made from fp32 q / k / v the way ff_ocab_attn rounds them: bf16(q * scale), bf16(k), bf16(v)."""
    B, H, W, _ = qkv32.shape
    perm = _perm(dev)
    real = perm >= 0
    s = torch.ones(576, device=dev)
    s[:192] = scale
    rows = torch.zeros(B, H, W, 576, device=dev, dtype=torch.bfloat16)
    rows[..., real] = (qkv32[..., perm[real]] * s[real]).bfloat16()
    return rows


@pytest.mark.parametrize("out_bf16", [True, False])
@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (1, 32, 48), (2, 32, 32)])
def test_attn_rows16_equals_fp32_rows_kernel(bf16_mode, dev, B, H, W, out_bf16):
    ops = bf16_mode
    scale = float(torch.tensor(D ** -0.5, dtype=torch.float32))
    qkv32 = rnd(B, H, W, 3 * C, dev=dev, seed=10 + H + W)
    rel = rnd(HEADS, 39 * 39, dev=dev, seed=11)

    def out_buf():
        return (ops.empty_rows_bf16((B, H, W, C), dev) if out_bf16 else ops.empty_rows((B, H, W, C), dev)).fill_(-3.0)

    want = ops.ocab_attn(qkv32, out_buf(), rel, q_off=0, k_off=C, v_off=2 * C, H=H, W=W, heads=HEADS, d=D, ws=16, ows=24, scale=scale)
    # 1e30 in the pad columns beyond 576 and in a guard row before and after: an over-read shows as a wrong result, not as a fault
    store = torch.full((B * H * W + 2, 640), 1e30, device=dev, dtype=torch.bfloat16)
    rows = store[1:-1].view(B, H, W, 640)[..., :576]
    rows.copy_(_padded_rows(qkv32, scale, dev))
    got = ops.ocab_attn_rows16(rows, out_buf(), rel, q_off=0, k_off=192, v_off=384, H=H, W=W, heads=HEADS, d=D, ws=16, ows=24)
    assert torch.isfinite(want.float()).all() and not torch.any(want == -3.0)
    assert torch.equal(got, want)


@pytest.fixture(scope="module")
def hat(dev, synth_sd):
    from isr2_amd.experts import HatHIP
    return HatHIP(synth_sd, "cuda:0")


def _old_chain(ops, hat, x, blk, mode):
    """The block as it was composed before the rows form: fp32 q / k / v rows between the projection and the attention."""
    from isr2_amd.prep import pack_token_linear, pack_token_projmlp
    _, H, W, _ = x.shape
    qkv = ops.token_linear(x, pack_token_linear(*blk["qkv"]), gamma=blk["n1"][0], beta=blk["n1"][1])
    if mode == "bf16":
        att = ops.empty_rows_bf16(tuple(x.shape), x.device)
        ops.ocab_attn(qkv, att, blk["rel"], q_off=0, k_off=C, v_off=2 * C, H=H, W=W, heads=HEADS, d=D, ws=16, ows=24, scale=D ** -0.5)
    else:
        att = ops.empty_like_rows(x)
        ops.window_attn(qkv, att, blk["bias"], q_off=0, k_off=C, v_off=2 * C, o_off=0, H=H, W=W, Hp=H, Wp=W, win=(16, 16), kwin=(24, 24),
                        shift=(0, 0), use_mask=False, heads=HEADS, d=D, scale=D ** -0.5)
    return ops.token_projmlp(att, x, pack_token_projmlp(*blk["proj"], *blk["fc1"], *blk["fc2"]), blk["n2"][0], blk["n2"][1])


@pytest.mark.parametrize("mode,B", [("bf16", 1), ("bf16", 2), ("bf16x3", 1), ("bf16x3", 2)])
def test_ocab_block_equals_old_chain(dev, hat, mode, B):
    from isr2_amd import ops
    old = ops.gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        blk = hat.ocab[1]
        x = ops.empty_rows((B, 32, 48, C), dev)
        x.copy_(rnd(B, 32, 48, C, dev=dev, seed=20 + B))
        calls = []
        real16 = ops.token_linear_rows16

        def counted(*a, **k):
            calls.append(1)
            return real16(*a, **k)

        ops.token_linear_rows16 = counted
        try:
            got = hat.ocab_block(x, blk)
        finally:
            ops.token_linear_rows16 = real16
        assert len(calls) == (1 if mode == "bf16" else 0)            # the rows route in plain bf16 only, one launch whatever B
        want = _old_chain(ops, hat, x, blk, mode)
        assert torch.isfinite(want).all()
        assert torch.equal(got, want)
    finally:
        ops.set_gemm_mode(old)
