"""The operand vocabulary of isr2_amd.ops, the parts that need no GPU: every pointer of ops.py is taken inside an operand helper (an AST
check), bf16 is accepted by a dtype argument and not by a name suffix, the instrumented set is the one bench.py's per-kernel-class
breakdown keys on, and every helper refuses a CPU tensor with an FFError that begins with the operand's name.  (The collapse rule of
rows_view cannot be reached with CPU tensors, the device check comes first: tests/test_ops_operands_gpu.py has it.)"""
import ast
import inspect

import pytest
import torch

# the only functions / classes of ops.py in which the attribute `data_ptr` may occur
POINTER_HELPERS = {"_rows", "_dense", "_out", "PoolPartials"}

INSTRUMENTED = {
    "conv2d", "cab_fused", "sgfn_tail", "ocab_attn", "ocab_attn_rows16", "token_linear_rows16", "linear", "win_attn_fused",
    "token_projmlp", "hab_link", "token_linear_gated", "token_mlp", "token_linear", "pixel_mlp", "dwconv3_gate_pool", "naf_front",
    "naf_ffn", "naf_tail", "window_attn", "layernorm", "pool_mean", "vec_mlp", "dwconv2d", "dwconv3x3_ln", "mix2", "fma3", "affine",
    "nchw_to_nhwc", "nhwc_to_nchw", "resize", "avgpool2", "dct8_bands", "dwt_pass", "fft_bands", "chan_attn_weights", "chan_qkv_attn",
    "band_mha_core", "band_weight", "freq_guidance", "dynamic_gates", "fuse_blend", "tile_accum", "tile_normalize"}


def _source():
    from isr2_amd import ops
    return inspect.getsource(ops)


def test_data_ptr_only_inside_the_operand_helpers():
    tree = ast.parse(_source())
    found = {}
    for top in tree.body:
        owner = top.name if isinstance(top, (ast.FunctionDef, ast.ClassDef)) else "<module>"
        for node in ast.walk(top):
            if (isinstance(node, ast.Attribute) and node.attr == "data_ptr") or (isinstance(node, ast.Name) and node.id == "data_ptr"):
                found.setdefault(owner, []).append(node.lineno)
    assert found, "ops.py takes no pointer at all: the check looks at the wrong file"
    assert set(found) <= POINTER_HELPERS, {k: v for k, v in found.items() if k not in POINTER_HELPERS}


def test_no_dtype_by_name_suffix():
    src = _source()
    assert "bf16ok" not in src
    for gone in ("def _chk(", "def _ptr(", "def _dense_out("):
        assert gone not in src, gone


def test_instrumented_set_and_names():
    assert len(INSTRUMENTED) == 43
    from isr2_amd import ops
    got = {n for n, f in vars(ops).items() if inspect.isfunction(f) and hasattr(f, "__wrapped__")}
    assert got == INSTRUMENTED, (sorted(got - INSTRUMENTED), sorted(INSTRUMENTED - got))
    for n in INSTRUMENTED:
        assert getattr(ops, n).__name__ == n and getattr(ops, n).__wrapped__.__name__ == n


def test_instrumentation_sits_at_the_definitions():
    tree = ast.parse(_source())
    decorated = {f.name for f in tree.body if isinstance(f, ast.FunctionDef)
                 and any(isinstance(d, ast.Name) and d.id == "_instrument" for d in f.decorator_list)}
    assert decorated == INSTRUMENTED
    assert "globals()" not in _source()


def _helper_calls():
    from isr2_amd import ops
    t = torch.zeros(2, 4, 4, 8)
    return {
        "_rows": lambda n: ops._rows(t, n),
        "_rows/bf16": lambda n: ops._rows(t.bfloat16(), n, dtype=ops._F32_BF16),
        "rows_view": lambda n: ops.rows_view(t, n),
        "_nhwc": lambda n: ops._nhwc(t, n, (2, 4, 4, 8)),
        "_dense/n": lambda n: ops._dense(torch.zeros(8), n, n=8),
        "_dense/shape": lambda n: ops._dense(t, n, shape=(2, None, 4, 8)),
        "_dense/u8": lambda n: ops._dense(torch.zeros(4, 4, 3, dtype=torch.uint8), n, ops._U8, shape=(None, None, 3)),
        "_image": lambda n: ops._image(torch.zeros(3, 5, dtype=torch.bfloat16), n),
        "_images": lambda n: ops._images({"w": torch.zeros(3)}, n[:-2], "w"),
        "_out/rows": lambda n: ops._out(t, n, (2, 4, 4, 8), "cpu"),
        "_out/nhwc": lambda n: ops._out(t, n, (2, 4, 4, 8), "cpu", kind="nhwc"),
        "_out/dense": lambda n: ops._out(t, n, (2, 4, 4, 8), "cpu", kind="dense"),
    }


@pytest.mark.parametrize("helper", ["_rows", "_rows/bf16", "rows_view", "_nhwc", "_dense/n", "_dense/shape", "_dense/u8", "_image", "_images",
                                    "_out/rows", "_out/nhwc", "_out/dense"])
def test_cpu_tensor_is_refused_by_name(helper):
    from isr2_amd.lib import FFError
    with pytest.raises(FFError) as ei:
        _helper_calls()[helper]("someop.operand.w")
    assert str(ei.value).startswith("someop.operand.w: "), str(ei.value)
    assert "CUDA(HIP)" in str(ei.value)


@pytest.mark.parametrize("bad", [None, 3.0, [1.0, 2.0]])
def test_non_tensor_is_refused_by_name(bad):
    from isr2_amd import ops
    from isr2_amd.lib import FFError
    for call in (lambda: ops._rows(bad, "op.x"), lambda: ops._nhwc(bad, "op.x"), lambda: ops._dense(bad, "op.x", n=2),
                 lambda: ops._image(bad, "op.x")):
        with pytest.raises(FFError, match=r"^op\.x: "):
            call()


def test_optional_operands():
    from isr2_amd import ops
    assert ops._rows(None, "op.res", 4, 8, optional=True) == (None, 0)
    assert ops._nhwc(None, "op.res", (1, 2, 2, 8), optional=True) == (None, 0)
    assert ops._dense(None, "op.bias", n=8, optional=True) is None
    assert ops._image(None, "op.pk.b", optional=True) is None


def test_wrappers_refuse_cpu_operands_before_the_library(monkeypatch):
    """No library on this path: _L raises if a wrapper reaches it."""
    from isr2_amd import ops
    from isr2_amd.lib import FFError

    def reached():
        raise AssertionError("reached the library")
    monkeypatch.setattr(ops, "_L", reached)
    x = torch.zeros(256, 180)
    g = torch.zeros(180)
    with pytest.raises(FFError, match=r"^layernorm\.x: "):
        ops.layernorm(x, g, g)
    with pytest.raises(FFError, match=r"^affine\.x: "):
        ops.affine(x, g, g)
    with pytest.raises(FFError, match=r"^tile_normalize\.acc: "):
        ops.tile_normalize(torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, 4))
    with pytest.raises(FFError, match=r"^band_weight\.x: "):
        ops.band_weight(torch.zeros(4, 27), torch.zeros(4, 9), torch.zeros(9))
    with pytest.raises(FFError, match=r"^fuse_blend\.experts9: "):
        ops.fuse_blend(torch.zeros(1, 8, 8, 9), torch.zeros(1, 8, 8, 3), torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3),
                       torch.zeros(1, 2, 2, 1))
