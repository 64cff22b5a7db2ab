"""HAT OCAB on head-padded bf16 rows, the parts that need no GPU: prep.pack_ocab_qkv's layout (a permuted, padded
pack_token_linear image plus the column scale) and the argument checks of ff_token_linear_rows16 / ff_ocab_attn_rows16, which refuse
before any launch."""
import numpy as np
import torch

HEADS, D, K = 6, 30, 180
C = HEADS * D


def _qkv(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3 * C, K, generator=g), torch.randn(3 * C, generator=g)


def test_pack_ocab_qkv_layout():
    from isr2_amd.prep import pack_ocab_qkv, pack_token_linear
    w, b = _qkv()
    pk = pack_ocab_qkv(w, b, HEADS, D)
    assert (pk["N"], pk["nt"], pk["K"], pk["kpad"]) == (576, 18, K, 192)
    # the tile image is pack_token_linear's of the permuted, padded matrix: rebuild that matrix column by column from the statement
    # "column 32 t + j (j < 30) carries the weight row and bias of q / k / v channel 30 (t % 6) + j", pad rows zero
    wp, bp = torch.zeros(576, K), torch.zeros(576)
    for t in range(18):
        part, head = t // HEADS, t % HEADS
        for j in range(D):
            wp[32 * t + j] = w[part * C + D * head + j]
            bp[32 * t + j] = b[part * C + D * head + j]
    want = pack_token_linear(wp, bp)
    assert torch.equal(pk["w"].view(torch.int16), want["w"].view(torch.int16)) and torch.equal(pk["b"], want["b"])
    # pad rows / biases are zero in the image itself: tile t, both planes, rows 30 and 31
    img = pk["w"].reshape(18, 2, 32, 192).float()
    assert torch.count_nonzero(img[:, :, 30:]) == 0 and torch.count_nonzero(pk["b"].reshape(18, 32)[:, 30:]) == 0
    assert torch.count_nonzero(img[:, 0, :30, :K]) > 0
    # the hi plane of a real row is the bf16 rounding of its weight row
    assert torch.equal(img[7, 0, 3, :K], w[C + D * 1 + 3].bfloat16().float())


def test_pack_ocab_qkv_scale():
    from isr2_amd.prep import pack_ocab_qkv
    pk = pack_ocab_qkv(*_qkv(1), HEADS, D)
    s = pk["scale"]
    assert s.dtype == torch.float32 and tuple(s.shape) == (576,)
    assert np.array_equal(s[:192].numpy(), np.full(192, np.float32(30 ** -0.5), dtype=np.float32))
    assert np.array_equal(s[192:].numpy(), np.ones(384, dtype=np.float32))


def test_pack_ocab_qkv_without_bias():
    from isr2_amd.prep import pack_ocab_qkv
    pk = pack_ocab_qkv(_qkv(2)[0], None, HEADS, D)
    assert torch.count_nonzero(pk["b"]) == 0 and tuple(pk["b"].shape) == (576,)


def _tl16(lib, **kw):
    a = dict(x=16, ldx=192, out=32, ldo=576, M=300, K=180, kpad=192, N=576, nt=18, gamma=None, beta=None, w=48, bias=64, scale=80, act=0,
             res=None, res2=None, rs2=None, xn=None, stats=None, nterms=1)
    a.update(kw)
    return lib.ff_token_linear_rows16(a["x"], a["ldx"], a["out"], a["ldo"], a["M"], a["K"], a["kpad"], a["N"], a["nt"], a["gamma"], a["beta"], 1e-5,
                                      a["w"], a["bias"], a["scale"], a["act"], a["res"], 576, a["res2"], 576, a["rs2"], a["xn"], 192,
                                      a["stats"], 0, 0, 1e-5, a["nterms"], None)


def test_token_linear_rows16_refusals():
    from isr2_amd import lib as L
    lib = L.load()
    for kw in (dict(nterms=3), dict(nterms=2), dict(act=1), dict(res=96), dict(res2=96, rs2=112), dict(xn=96), dict(stats=96)):
        assert _tl16(lib, **kw) != 0, kw
        assert b"ff_token_linear_rows16: plain bf16" in lib.ff_last_error(), kw
    for kw, msg in ((dict(ldo=578), b"8-byte aligned"), (dict(ldo=572), b"8-byte aligned"), (dict(out=36), b"8-byte aligned"),
                    (dict(scale=None), b"null pointer"), (dict(scale=84), b"16-byte aligned"), (dict(N=578, nt=19), b"multiples of 4"),
                    (dict(kpad=160), b"kpad"), (dict(nt=17), b"n_tiles")):
        assert _tl16(lib, **kw) != 0, kw
        assert msg in lib.ff_last_error(), (kw, lib.ff_last_error())


def _oc16(lib, **kw):
    a = dict(qkv=64, ldq=576, q=0, k=192, v=384, out=128, ldo=192, o=0, rel=256, B=1, H=32, W=48, heads=6, d=30, ws=16, ows=24)
    a.update(kw)
    return lib.ff_ocab_attn_rows16(a["qkv"], a["ldq"], a["q"], a["k"], a["v"], a["out"], a["ldo"], a["o"], a["rel"], a["B"], a["H"], a["W"],
                                   a["heads"], a["d"], a["ws"], a["ows"], 1, None)


def test_ocab_attn_rows16_refusals():
    from isr2_amd import lib as L
    lib = L.load()
    for kw, msg in ((dict(ldq=580), b"16-byte aligned"), (dict(qkv=72), b"16-byte aligned"), (dict(k=180), b"multiples of 32"),
                    (dict(v=360), b"multiples of 32"), (dict(q=30), b"multiples of 32"), (dict(v=416), b"rows too short"),
                    (dict(ldq=544), b"rows too short"), (dict(d=32), b"head dim 30"), (dict(H=40), b"multiples of the window"),
                    (dict(qkv=None), b"null pointer"), (dict(ldo=176), b"hold every head")):
        assert _oc16(lib, **kw) != 0, kw
        assert msg in lib.ff_last_error(), (kw, lib.ff_last_error())
