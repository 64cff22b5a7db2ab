"""ops.hab_link (csrc/hab_link.hip): one HAB's token_projmlp and the next HAB's win_attn_fused in one launch, against the two launches,
bit for bit (torch.equal on x_out fp32, xn bf16 and att bf16: the link runs the parents' statements in their order, so there is no
tolerance), and HatHIP.group -- which uses the link between the blocks of a group in plain bf16 -- against the per-block loop.

Shapes: 32 x 32 is four 16 x 16 windows; with shift 8 three of them are masked and one is not, the smallest case that has both.
48 x 32 is not square (the row / column wrap of the shift and the window grid differ).  B = 2 carries one gate row per image."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

C, HEADS, D, WS = 180, 6, 30, 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rnd(*shape, dev, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


class _Mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from isr2_amd import ops
        self.prev = ops.gemm_mode()
        ops.set_gemm_mode(self.mode)
        return ops

    def __exit__(self, *exc):
        from isr2_amd import ops
        ops.set_gemm_mode(self.prev)


@pytest.fixture(scope="module")
def weights(dev):
    from isr2_amd.prep import pack_token_projmlp, pack_win_attn, pack_win_rel
    Hd = 2 * C
    pm = pack_token_projmlp(rnd(C, C, dev=dev, seed=1950, scale=1.0 / math.sqrt(C)), rnd(C, dev=dev, seed=1951, scale=0.1),
                            rnd(Hd, C, dev=dev, seed=1952, scale=1.0 / math.sqrt(C)), rnd(Hd, dev=dev, seed=1953, scale=0.1),
                            rnd(C, Hd, dev=dev, seed=1954, scale=1.0 / math.sqrt(Hd)), rnd(C, dev=dev, seed=1955, scale=0.1))
    wf = pack_win_attn(rnd(3 * C, C, dev=dev, seed=1956, scale=1.0 / math.sqrt(C)), rnd(3 * C, dev=dev, seed=1957, scale=0.1), HEADS, D, D ** -0.5)
    relp = pack_win_rel(rnd(HEADS, (2 * WS - 1) ** 2, dev=dev, seed=1958, scale=0.5).contiguous(), WS, WS)
    n2 = ((rnd(C, dev=dev, seed=1959) * 0.1 + 1).contiguous(), (rnd(C, dev=dev, seed=1960) * 0.1).contiguous())
    n1 = ((rnd(C, dev=dev, seed=1961) * 0.1 + 1).contiguous(), (rnd(C, dev=dev, seed=1962) * 0.1).contiguous())
    return dict(pm=pm, wf=wf, relp=relp, n1=n1, n2=n2)


def _rows(B, H, W, dev, seed, bf16):
    from isr2_amd import ops
    t = ops.empty_rows_bf16((B, H, W, C), dev) if bf16 else ops.empty_rows((B, H, W, C), dev)
    t.copy_(rnd(B, H, W, C, dev=dev, seed=seed))
    return t


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("shift", [0, 8])
@pytest.mark.parametrize("H,W", [(32, 32), (48, 32)])
def test_hab_link_equals_projmlp_then_attention(dev, weights, H, W, shift, B):
    w = weights
    with _Mode("bf16") as ops:
        att, c2 = _rows(B, H, W, dev, 1970, True), _rows(B, H, W, dev, 1971, True)
        x = _rows(B, H, W, dev, 1972, False)
        gate = (torch.sigmoid(rnd(B, C, dev=dev, seed=1973)) * 0.01).contiguous()          # one row per image, all different
        if B == 1:
            gate = gate.reshape(-1)
        else:
            assert not torch.equal(gate[0], gate[1])
        x_ref = ops.token_projmlp(att, x, w["pm"], *w["n2"], c2=c2, c2_scale=gate)
        att_ref = ops.empty_rows_bf16((B, H, W, C), dev)
        _, xn_ref = ops.win_attn_fused(x_ref, att_ref, w["wf"], w["relp"], gamma=w["n1"][0], beta=w["n1"][1], H=H, W=W, Hp=H, Wp=W,
                                       win=(WS, WS), shift=(shift, shift), use_mask=shift > 0, want_xn="bf16")
        x_out, xn, att_out = ops.hab_link(att, x, w["pm"], *w["n2"], c2=c2, c2_scale=gate, wf=w["wf"], rel_padded=w["relp"],
                                          gamma1=w["n1"][0], beta1=w["n1"][1], shift=(shift, shift), use_mask=shift > 0)
        torch.cuda.synchronize()
        assert x_out.dtype == torch.float32 and xn.dtype == torch.bfloat16 and att_out.dtype == torch.bfloat16
        assert tuple(x_out.shape) == tuple(xn.shape) == tuple(att_out.shape) == (B, H, W, C)
        assert torch.isfinite(x_ref).all() and torch.isfinite(att_ref.float()).all()
        assert torch.equal(x_out, x_ref), f"x_out: max diff {(x_out - x_ref).abs().max().item():.3e}"
        assert torch.equal(xn, xn_ref), f"xn: max diff {(xn.float() - xn_ref.float()).abs().max().item():.3e}"
        assert torch.equal(att_out, att_ref), f"att: max diff {(att_out.float() - att_ref.float()).abs().max().item():.3e}"
        if B == 2:                                                       # the gate row is the image's own
            assert not torch.equal(x_out[0], x_out[1])


def test_hab_link_needs_plain_bf16(dev, weights):
    from isr2_amd.lib import FFError
    w = weights
    with _Mode("bf16x3") as ops:
        att, c2, x = _rows(1, 32, 32, dev, 1970, True), _rows(1, 32, 32, dev, 1971, True), _rows(1, 32, 32, dev, 1972, False)
        with pytest.raises(FFError):
            ops.hab_link(att, x, w["pm"], *w["n2"], c2=c2, c2_scale=torch.zeros(C, device=dev), wf=w["wf"], rel_padded=w["relp"],
                         gamma1=w["n1"][0], beta1=w["n1"][1], shift=(0, 0), use_mask=False)


# ---- HatHIP.group ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hat(dev, synth_sd):
    from isr2_amd.experts import HatHIP
    return HatHIP(synth_sd, dev)


def _loop(hat, ops, x, g):
    y = x
    for blk in hat.blocks[g]:
        y = hat.hab(y, blk)
    y = hat.ocab_block(y, hat.ocab[g])
    return ops.conv2d(y, *hat.gconv[g], ksize=(3, 3), pad=(1, 1), res=x, per_image=True)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("H,W", [(32, 32), (48, 32)])
def test_group_equals_the_per_block_loop_in_plain_bf16(dev, hat, H, W, B):
    with _Mode("bf16") as ops:
        x = _rows(B, H, W, dev, 1980, False)
        want = _loop(hat, ops, x, 0)
        with ops.profile() as prof:
            got = hat.group(x, 0)
        names = [r[0] for r in prof.records()]
        assert names.count("hab_link") == 5 and names.count("win_attn_fused") == 1 and names.count("token_projmlp") == 2, names   # (one of the two is OCAB's)
        assert torch.isfinite(want).all()
        assert torch.equal(got, want), f"max diff {(got - want).abs().max().item():.3e}"


def test_group_keeps_its_launches_in_bf16x3(dev, hat):
    with _Mode("bf16x3") as ops:
        x = _rows(1, 32, 32, dev, 1981, False)
        with ops.profile() as prof:
            want = _loop(hat, ops, x, 0)
        loop_names = [r[0] for r in prof.records()]
        with ops.profile() as prof:
            got = hat.group(x, 0)
        names = [r[0] for r in prof.records()]
        assert names == loop_names and "hab_link" not in names, names
        assert torch.equal(got, want)
