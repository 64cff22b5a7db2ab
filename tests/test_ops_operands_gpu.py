"""The operand vocabulary of isr2_amd.ops on device tensors.  Nothing here launches a kernel of the library: ops._L is replaced by a proxy
whose every attribute access raises AssertionError("reached the library"), so a case either is refused with an FFError first -- the
thing under test -- or stops at the proxy.

For every wrapper that used to hand small operands (LayerNorm vectors, tap weights, statistics, temperatures, tables) to the library
unchecked: valid operands at the smallest legal shape reach the proxy, and with ONE small operand replaced by (a) a CPU tensor, (b) the
same values as float64, (c) a strided view with the right element count, (d) one element too few, the call raises FFError naming
"op.operand".  bf16 rows are accepted exactly where a kernel reads them; the collapse rule of the rows helper is pinned against values
written from the strides."""
import pytest
import torch

pytestmark = pytest.mark.gpu

REACHED = "reached the library"


@pytest.fixture()
def ops(monkeypatch):
    from isr2_amd import ops as O

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(REACHED)

    monkeypatch.setattr(O, "_L", lambda: NoLaunch())
    prev = O.gemm_mode()
    O.set_gemm_mode("bf16")                       # the one mode in which every wrapper below exists
    yield O
    O.set_gemm_mode(prev)


def z(*shape, dtype=torch.float32):
    return torch.zeros(shape, device="cuda", dtype=dtype)


def _img():
    return z(8, dtype=torch.bfloat16)             # a prepared image: the helpers ask for a contiguous device tensor, nothing else


def _mlp_pk():
    return {"K": 180, "N": 180, "ht": 23, "w": _img(), "b1": z(8), "b2": z(8)}


# op -> (valid operands, call, {operand key: (name in the message, mutations)}); "abcd" = all four replacements.  Where the element
# count an operand must have is derived from that operand itself (band_weight.x, ...), "one element too few" has no meaning: "abc".
def _cases():
    tl_pk = {"K": 180, "N": 180, "kpad": 192, "nt": 6, "w": _img(), "b": z(8)}
    return {
        "layernorm": (dict(x=z(256, 180), gamma=z(180), beta=z(180)),
                      lambda o, d: o.layernorm(d["x"], d["gamma"], d["beta"]), {"gamma": "abcd", "beta": "abcd"}),
        "affine": (dict(x=z(256, 180), scale=z(180), shift=z(180)),
                   lambda o, d: o.affine(d["x"], d["scale"], d["shift"]), {"scale": "abcd", "shift": "abcd"}),
        "token_mlp": (dict(x=z(256, 180), gamma=z(180), beta=z(180)),
                      lambda o, d: o.token_mlp(d["x"], d["gamma"], d["beta"], _mlp_pk()), {"gamma": "abcd", "beta": "abcd"}),
        "token_projmlp": (dict(att=z(256, 180), x=z(256, 180), gamma=z(180), beta=z(180), c2=z(256, 180), c2_scale=z(180)),
                          lambda o, d: o.token_projmlp(d["att"], d["x"], {"mlp": _mlp_pk(), "proj": {"w": _img(), "b": z(8)}}, d["gamma"],
                                                       d["beta"], c2=d["c2"], c2_scale=d["c2_scale"]),
                          {"gamma": "abcd", "beta": "abcd", "c2_scale": "abcd"}),
        "token_linear": (dict(x=z(256, 180), gamma=z(180), beta=z(180), res2=z(256, 180), res2_scale=z(180)),
                         lambda o, d: o.token_linear(d["x"], tl_pk, gamma=d["gamma"], beta=d["beta"], res2=d["res2"],
                                                     res2_scale=d["res2_scale"]),
                         {"gamma": "abcd", "beta": "abcd", "res2_scale": "abcd"}),
        "chan_qkv_attn": (dict(x=z(256, 180), gamma=z(180), beta=z(180), temperature=z(6, 1, 1)),
                          lambda o, d: o.chan_qkv_attn(d["x"], {"K": 180, "w": _img(), "b": z(8)}, d["gamma"], d["beta"], d["temperature"]),
                          {"gamma": "abcd", "beta": "abcd", "temperature": "abcd"}),
        "naf_front": (dict(x=z(1, 16, 16, 64), ln_g=z(64), ln_b=z(64), w_tap=z(9, 128), dw_bias=z(128)),
                      lambda o, d: o.naf_front(d["x"], {"N": 128, "K": 64, "kpad": 64, "w": _img(), "b": z(8)}, d["ln_g"], d["ln_b"],
                                               d["w_tap"], d["dw_bias"]),
                      {"ln_g": "abcd", "ln_b": "abcd", "w_tap": "abcd", "dw_bias": "abcd"}),
        "naf_ffn": (dict(y=z(1, 16, 16, 64), ln_g=z(64), ln_b=z(64), out_scale=z(64)),
                    lambda o, d: o.naf_ffn(d["y"], {"C": 64, "w": _img(), "b4": z(8), "b5": z(8)}, d["ln_g"], d["ln_b"], d["out_scale"]),
                    {"ln_g": "abcd", "ln_b": "abcd", "out_scale": "abcd"}),
        "dwconv3x3_ln": (dict(x=z(1, 16, 16, 32), w_tap=z(9, 32), bias=z(32), stats=z(256, 2), gamma=z(32), beta=z(32)),
                         lambda o, d: o.dwconv3x3_ln(d["x"], d["w_tap"], d["bias"], d["stats"], d["gamma"], d["beta"]),
                         {"w_tap": "abcd", "bias": "abcd", "stats": "abcd", "gamma": "abcd", "beta": "abcd"}),
        "sgfn_tail": (dict(y=z(1, 16, 16, 64), w_tap=z(9, 32), dw_bias=z(32), stats=z(256, 2), gamma=z(32), beta=z(32), w2=z(48, 32),
                           b2=z(48)),
                      lambda o, d: o.sgfn_tail(d["y"], 32, d["w_tap"], d["dw_bias"], d["stats"], d["gamma"], d["beta"], d["w2"], d["b2"]),
                      {"w_tap": "abcd", "dw_bias": "abcd", "stats": "abcd", "gamma": "abcd", "beta": "abcd", "b2": "abcd",
                       "w2": "abd"}),              # (w2 reaches the kernel as a repacked image: a strided one is read correctly)
        "pixel_mlp": (dict(x=z(256, 180), W1=z(8, 180), b1=z(8), w2=z(1, 8)),
                      lambda o, d: o.pixel_mlp(d["x"], d["W1"], d["b1"], "gelu", d["w2"], 0.5, "sigmoid"),
                      {"W1": "abc", "b1": "abcd", "w2": "abd"}),      # (the hidden width is W1's; a strided w2 is gathered by reshape(-1))
        "vec_mlp": (dict(v=z(1, 180), W1=z(6, 180), b1=z(6), W2=z(180, 6), b2=z(180)),
                    lambda o, d: o.vec_mlp(d["v"], d["W1"], d["b1"], "relu", d["W2"], d["b2"], "sigmoid"),
                    {"v": "abcd", "W1": "abcd", "b1": "abcd", "W2": "abcd", "b2": "abcd"}),
        "dct8_bands": (dict(x=z(3, 16, 16), dct_mat=z(8, 8), masks3=z(3, 8, 8), band_scale=z(3), out=z(1, 16, 16, 27)),
                       lambda o, d: o.dct8_bands(d["x"], d["dct_mat"], d["masks3"], d["band_scale"], d["out"], 0),
                       {"x": "abc", "dct_mat": "abcd", "masks3": "abcd", "band_scale": "abcd"}),
        "fft_bands": (dict(x=z(3, 16, 16), twW0=z(16), twW1=z(16), twH0=z(16), twH1=z(16), mask_logits=z(64, 64), band_scale2=z(2),
                           out=z(1, 16, 16, 27)),
                      lambda o, d: o.fft_bands(d["x"], (d["twW0"], d["twW1"]), (d["twH0"], d["twH1"]), d["mask_logits"], 1.0,
                                               d["band_scale2"], d["out"], 21, 24),
                      {"twW0": "abcd", "twW1": "abcd", "twH0": "abcd", "twH1": "abcd", "mask_logits": "abcd", "band_scale2": "abcd"}),
        "dwt_pass": (dict(x=z(3, 16, 16), lo8=z(8), hi8=z(8)),
                     lambda o, d: o.dwt_pass(d["x"], 1, d["lo8"], d["hi8"]), {"x": "abc", "lo8": "abcd", "hi8": "abcd"}),
        "band_weight": (dict(x=z(256, 27), att=z(256, 9), imp=z(9)),
                        lambda o, d: o.band_weight(d["x"], d["att"], d["imp"]), {"x": "abc", "att": "abcd", "imp": "abcd"}),
        "freq_guidance": (dict(b3=z(1, 16, 16, 9)), lambda o, d: o.freq_guidance(d["b3"]), {"b3": "abc"}),
        "dynamic_gates": (dict(graw=z(1, 16, 16, 3), dif=z(1, 16, 16, 1)),
                          lambda o, d: o.dynamic_gates(d["graw"], d["dif"]), {"graw": "abc", "dif": "abcd"}),
        "fuse_blend": (dict(experts9=z(1, 8, 8, 9), hier3=z(1, 8, 8, 3), guide3=z(1, 2, 2, 3), gates3=z(1, 2, 2, 3), dif1=z(1, 2, 2, 1)),
                       lambda o, d: o.fuse_blend(d["experts9"], d["hier3"], d["guide3"], d["gates3"], d["dif1"]),
                       {"experts9": "abcd", "hier3": "abcd", "guide3": "abcd", "gates3": "abcd", "dif1": "abcd"}),
        "tile_normalize": (dict(acc=z(1, 3, 8, 8), wsum=z(1, 1, 8, 8)),
                           lambda o, d: o.tile_normalize(d["acc"], d["wsum"]), {"acc": "abcd", "wsum": "abcd"}),
    }


OPS = ["layernorm", "affine", "token_mlp", "token_projmlp", "token_linear", "chan_qkv_attn", "naf_front", "naf_ffn", "dwconv3x3_ln",
       "sgfn_tail", "pixel_mlp", "vec_mlp", "dct8_bands", "fft_bands", "dwt_pass", "band_weight", "freq_guidance", "dynamic_gates",
       "fuse_blend", "tile_normalize"]
MESSAGE_NAME = {"twW0": "twW[0]", "twW1": "twW[1]", "twH0": "twH[0]", "twH1": "twH[1]"}


def _mutate(t, how):
    if how == "a":
        return t.cpu()
    if how == "b":
        return t.double()
    if how == "c":                                 # the right element count, every second element of a buffer twice as wide
        v = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), device=t.device, dtype=t.dtype)[..., ::2]
        assert v.shape == t.shape and not v.is_contiguous()
        return v
    return t.reshape(-1)[:-1]                      # "d": one element too few


def test_case_table_is_complete():
    assert sorted(_cases()) == sorted(OPS)


@pytest.mark.parametrize("op", OPS)
def test_valid_operands_reach_the_library(ops, op):
    valid, call, _ = _cases()[op]
    with pytest.raises(AssertionError, match=REACHED):
        call(ops, valid)


@pytest.mark.parametrize("op", OPS)
def test_small_operands_are_refused_by_name(ops, op):
    from isr2_amd.lib import FFError
    valid, call, small = _cases()[op]
    for key, hows in small.items():
        name = f"{op}.{MESSAGE_NAME.get(key, key)}"
        for how in hows:
            d = dict(valid)
            d[key] = _mutate(valid[key], how)
            with pytest.raises(FFError) as ei:
                call(ops, d)
            assert str(ei.value).startswith(name + ": "), f"{name} ({how}): {ei.value}"


# ---- bf16 rows: accepted where a kernel reads them, refused by the operand's name elsewhere ------------------------------------------
def _accepted(fn):
    with pytest.raises(AssertionError, match=REACHED):
        fn()


def _refused(fn, name):
    from isr2_amd.lib import FFError
    with pytest.raises(FFError) as ei:
        fn()
    assert str(ei.value).startswith(name + ": "), str(ei.value)


def test_bf16_by_helper(ops):
    r16, r32 = ops.empty_rows_bf16((1, 16, 16, 180), "cuda"), ops.empty_rows((1, 16, 16, 180), "cuda")
    assert ops._rows(r16, "op.x", dtype=ops._F32_BF16)[1:] == (192, 256, 180) and ops._rows(r16, "op.x", dtype=ops._BF16)[1] == 192
    assert ops._nhwc(r16, "op.x", dtype=ops._F32_BF16)[1:] == (192, 1, 16, 16, 180)
    _refused(lambda: ops._rows(r16, "op.x"), "op.x")
    _refused(lambda: ops.rows_view(r16, "op.x"), "op.x")
    _refused(lambda: ops._nhwc(r16, "op.x"), "op.x")
    _refused(lambda: ops._rows(r32, "op.x", dtype=ops._BF16), "op.x")
    _refused(lambda: ops._dense(z(8, dtype=torch.bfloat16), "op.gamma", n=8), "op.gamma")
    assert ops._image(z(8, dtype=torch.bfloat16), "op.pk.w") != 0
    out, p, ld = ops._out(None, "op.out", (256, 180), "cuda", bf16=True)
    assert out.dtype == torch.bfloat16 and ld == 192 and p == out.data_ptr()
    _refused(lambda: ops._out(r32, "op.out", (1, 16, 16, 180), "cuda", bf16=True), "op.out")
    _refused(lambda: ops._out(r16, "op.out", (1, 16, 16, 180), "cuda"), "op.out")
    _refused(lambda: ops._out(r16, "op.out", (1, 16, 16, 180), "cuda", bf16=True, kind="dense"), "op.out")     # padded pitch: not dense


def test_bf16_by_wrapper(ops):
    g = z(180)
    x32, x16 = ops.empty_rows((256, 180), "cuda"), ops.empty_rows_bf16((256, 180), "cuda")
    # layernorm: bf16 out with out_bf16, never a bf16 input
    _accepted(lambda: ops.layernorm(x32, g, g, out_bf16=True))
    _accepted(lambda: ops.layernorm(x32, g, g, out=x16, out_bf16=True))
    _refused(lambda: ops.layernorm(x16, g, g), "layernorm.x")
    # linear: bf16 rows into the rows GEMM (K % 64 == 0); res stays fp32
    a16, w = ops.empty_rows_bf16((256, 64), "cuda"), z(64, 64)
    _accepted(lambda: ops.linear(a16, w))
    _refused(lambda: ops.linear(a16, w, res=ops.empty_rows_bf16((256, 64), "cuda")), "linear.res")
    _refused(lambda: ops.linear(a16, w, bias=z(64, dtype=torch.bfloat16)), "linear.bias")
    # token_projmlp: att and c2 may be bf16 rows, x may not
    pk = {"mlp": _mlp_pk(), "proj": {"w": _img(), "b": z(8)}}
    _accepted(lambda: ops.token_projmlp(x16, x32, pk, g, g, c2=x16, c2_scale=g))
    _refused(lambda: ops.token_projmlp(x16, x16, pk, g, g, c2=x16, c2_scale=g), "token_projmlp.x")
    # ocab_attn: fp32 qkv, either out; ocab_attn_rows16: bf16 qkv only
    kw = dict(q_off=0, k_off=192, v_off=384, H=16, W=16, heads=6, d=30, ws=16, ows=24)
    q32, q16, rel = ops.empty_rows((1, 16, 16, 576), "cuda"), ops.empty_rows_bf16((1, 16, 16, 576), "cuda"), z(6, 39 * 39)
    o32, o16 = ops.empty_rows((1, 16, 16, 180), "cuda"), ops.empty_rows_bf16((1, 16, 16, 180), "cuda")
    _accepted(lambda: ops.ocab_attn(q32, o16, rel, scale=1.0, **kw))
    _accepted(lambda: ops.ocab_attn(q32, o32, rel, scale=1.0, **kw))
    _refused(lambda: ops.ocab_attn(q16, o16, rel, scale=1.0, **kw), "ocab_attn.qkv")
    _accepted(lambda: ops.ocab_attn_rows16(q16, o16, rel, **kw))
    _refused(lambda: ops.ocab_attn_rows16(q32, o16, rel, **kw), "ocab_attn_rows16.qkv")
    _refused(lambda: ops.ocab_attn(q32, o16, rel.double(), scale=1.0, **kw), "ocab_attn.rel_rotated")
    _refused(lambda: ops.ocab_attn(q32, o16, rel.bfloat16(), scale=1.0, **kw), "ocab_attn.rel_rotated")
    _refused(lambda: ops.ocab_attn_rows16(q16, o16, rel.double(), **kw), "ocab_attn_rows16.rel_rotated")
    # window_attn (split-bf16 route): the relative-position tables are fp32, equal windows and overlapping keys alike
    akw = dict(q_off=0, k_off=192, v_off=384, o_off=0, H=16, W=16, Hp=16, Wp=16, win=(16, 16), shift=(0, 0), use_mask=False, heads=6,
               d=30, scale=1.0)
    for kwin, nrel in (((16, 16), 31 * 31), ((24, 24), 39 * 39)):
        bT, tab = z(6, kwin[0] * kwin[1], 256), z(6, nrel)
        _accepted(lambda: ops.window_attn(q32, o32, bT, kwin=kwin, rel_table=tab, **akw))
        _refused(lambda: ops.window_attn(q32, o32, bT, kwin=kwin, rel_table=tab.double(), **akw), "window_attn.rel_table")
        _refused(lambda: ops.window_attn(q32, o32, bT.double(), kwin=kwin, rel_table=tab, **akw), "window_attn.biasT")
    # win_attn_fused: bf16 out / xn, fp32 x
    wf = {"K": 180, "heads": 6, "d": 30, "w": _img(), "b": z(8)}
    relp = z(6, 31, 32)
    wkw = dict(gamma=g, beta=g, H=16, W=16, Hp=16, Wp=16, win=(16, 16), shift=(0, 0), use_mask=False)
    x4 = ops.empty_rows((1, 16, 16, 180), "cuda")
    _accepted(lambda: ops.win_attn_fused(x4, o16, wf, relp, want_xn="bf16", **wkw))
    _refused(lambda: ops.win_attn_fused(o16, o16, wf, relp, **wkw), "win_attn_fused.x")
    _refused(lambda: ops.win_attn_fused(x4, o16, wf, relp.double(), **wkw), "win_attn_fused.rel_padded")
    # hab_link and cab_fused read bf16 rows only
    hkw = dict(c2=o16, c2_scale=g, wf=wf, rel_padded=relp, gamma1=g, beta1=g, shift=(0, 0), use_mask=False)
    _accepted(lambda: ops.hab_link(o16, x4, pk, g, g, **hkw))
    _refused(lambda: ops.hab_link(x4, x4, pk, g, g, **hkw), "hab_link.att")
    _refused(lambda: ops.hab_link(o16, o16, pk, g, g, **hkw), "hab_link.x")
    _refused(lambda: ops.hab_link(o16, x4, pk, g, g, **dict(hkw, rel_padded=relp.double())), "hab_link.rel_padded")
    _refused(lambda: ops.cab_fused(x4, (z(60, 9 * 180), z(60)), (z(180, 9 * 60), z(180))), "cab_fused.xn")
    # conv2d: bf16 x / out in the plain-bf16 LDS-resident 3x3 form; its residual stays fp32
    c16, cw = ops.empty_rows_bf16((1, 32, 32, 64), "cuda"), z(64, 9 * 64)
    _accepted(lambda: ops.conv2d(c16, cw, ksize=(3, 3), pad=(1, 1), out_bf16=True))
    _refused(lambda: ops.conv2d(ops.empty_rows((1, 32, 32, 64), "cuda"), cw, ksize=(3, 3), pad=(1, 1),
                                res=ops.empty_rows_bf16((1, 32, 32, 64), "cuda")), "conv2d.res")


# ---- the collapse rule ---------------------------------------------------------------------------------------------------------------
def test_rows_collapse_rule(ops):
    from isr2_amd.lib import FFError
    dense = z(4, 6, 180)
    assert ops._rows(dense, "t") == (dense.data_ptr(), 180, 24, 180) == ops.rows_view(dense, "t")
    buf = ops.empty_rows((2, 8, 8, 180), "cuda")                       # pitch 192 floats
    assert buf.stride() == (8 * 8 * 192, 8 * 192, 192, 1)
    sl = buf[..., 30:90]
    want = (buf.data_ptr() + 4 * 30, 192, 2 * 8 * 8, 60)
    assert ops._rows(sl, "t") == want == ops.rows_view(sl, "t")
    assert ops._rows(sl, "t", rows=128, C=60) == want
    assert ops._nhwc(sl, "t", (2, 8, 8, 60)) == (want[0], 192, 2, 8, 8, 60)
    b16 = ops.empty_rows_bf16((256, 180), "cuda")[:, 64:128]           # pitch 192 bf16 elements, 2 bytes each
    assert ops._rows(b16, "t", dtype=ops._BF16) == (b16.data_ptr(), 192, 256, 64) and b16.data_ptr() % 128 == 0
    vec = z(180)
    assert ops._rows(vec, "t") == (vec.data_ptr(), 180, 1, 180)       # a vector is one row
    one = z(5, 1, 7, 180)                                              # extents of 1 carry no stride
    assert ops._rows(one, "t") == (one.data_ptr(), 180, 35, 180)
    crop = z(2, 8, 10, 64)[:, :, :8]                                   # W cropped: rows of one image row follow each other, image rows do not
    for fn in (lambda: ops._rows(crop, "op.x"), lambda: ops.rows_view(crop, "op.x"), lambda: ops._nhwc(crop, "op.x")):
        with pytest.raises(FFError, match=r"^op\.x: leading dims do not collapse"):
            fn()
    with pytest.raises(FFError, match=r"^op\.x: last dim must be contiguous"):
        ops._rows(z(8, 360)[:, ::2], "op.x")
    with pytest.raises(FFError, match=r"^op\.x: last dim must be contiguous"):
        ops._rows(z(360)[::2], "op.x")
    for kw in (dict(rows=127), dict(C=64)):
        with pytest.raises(FFError, match=r"^op\.x: shape mismatch"):
            ops._rows(sl, "op.x", **kw)
    with pytest.raises(FFError, match=r"^op\.x: shape"):
        ops._nhwc(sl, "op.x", (2, 8, 8, 64))
    with pytest.raises(FFError, match=r"^op\.x: expected \[B,H,W,C\]"):
        ops._nhwc(dense, "op.x")
