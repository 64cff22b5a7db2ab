"""Operand-rounded fp64 references for the plain-bf16 ('bf16') and 'bf16x2' contraction modes (pure torch, CPU or GPU).

The bf16 MFMA multiplies its bf16 operands exactly and accumulates in fp32, so a reference that rounds the operands the way the
kernel's staging path does and multiplies in fp64 differs from a correct kernel by fp32-accumulation error only -- the operand
rounding itself (about 2.5e-3 of max|ref|) cancels.  tests/test_lowprec_ref.py checks this module on the CPU;
tests/test_lowprec_exact_gpu.py compares the kernels with it."""
import torch
import torch.nn.functional as F

FP32_CHAIN_TOL = 2e-5      # of max(1, max|ref|): the project's bound for an fp32 accumulation chain (GEMM_TOL["f32"] in test_ops_gpu.py)


def bf16_rne(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> the nearest bf16 value (ties to even), returned as fp32.  Integer arithmetic on the bit pattern (finite inputs), so it
    does not lean on the conversion it is used to check."""
    assert x.dtype == torch.float32
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u)
    return u.to(torch.int32).view(torch.float32).reshape(x.shape)


def bf16_trunc(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits (what a kernel that forgets to round computes), as fp32."""
    assert x.dtype == torch.float32
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).reshape(x.shape)


def split_bf16x2(x: torch.Tensor) -> torch.Tensor:
    """The A operand of 'bf16x2' as the staging path builds it: hi + lo with hi = rne(x), lo = rne(x - hi); fp64."""
    hi = bf16_rne(x)
    lo = bf16_rne(x - hi)                    # x - hi is exact in fp32
    return hi.double() + lo.double()


def operand_a(x: torch.Tensor, mode: str, kmul: torch.Tensor = None) -> torch.Tensor:
    """fp64 image of the activation operand: kmul (per input channel) is applied first, in fp32 -- one IEEE multiply, as in the kernel."""
    xs = x.float() if kmul is None else x.float() * kmul
    if mode == "bf16":
        return bf16_rne(xs).double()
    if mode == "bf16x2":
        return split_bf16x2(xs)
    raise ValueError(mode)


def operand_w(w: torch.Tensor) -> torch.Tensor:
    """fp64 image of the weight operand of both modes: the hi plane alone."""
    return bf16_rne(w.float()).double()


def conv_taps_f64(a: torch.Tensor, w: torch.Tensor, stride: int = 1, pad: int = 0) -> torch.Tensor:
    """Convolution as a sum over filter taps of shifted fp64 matmuls (needs no fp64 convolution backend).
    a [B, H, W, Cin] fp64 (NHWC), w [Cout, Cin, KH, KW] fp64 -> [B, Ho, Wo, Cout] fp64."""
    assert a.dtype == torch.float64 and w.dtype == torch.float64
    B, H, W, Cin = a.shape
    Cout, Cin2, KH, KW = w.shape
    assert Cin == Cin2
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    ap = F.pad(a, (0, 0, pad, pad, pad, pad)) if pad else a
    out = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float64, device=a.device)
    for ky in range(KH):
        for kx in range(KW):
            sl = ap[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride, :]
            out += sl.reshape(-1, Cin).matmul(w[:, :, ky, kx].t()).reshape(B, Ho, Wo, Cout)
    return out


def act_f64(y: torch.Tensor, act, gelu: str = "erf") -> torch.Tensor:
    assert y.dtype == torch.float64
    if act is None:
        return y
    if act == "gelu":
        return F.gelu(y, approximate="tanh") if gelu == "tanh" else 0.5 * y * (1.0 + torch.erf(y * 0.7071067811865476))
    if act == "relu":
        return torch.relu(y)
    if act == "lrelu":
        return torch.where(y > 0, y, 0.01 * y)
    if act == "sigmoid":
        return torch.sigmoid(y)
    raise ValueError(act)


def pixel_shuffle2_nhwc(y: torch.Tensor) -> torch.Tensor:
    """[B, H, W, 4 C] -> [B, 2 H, 2 W, C] with input channel 4 c + 2 dy + dx -> pixel (2 y + dy, 2 x + dx): nn.PixelShuffle(2)."""
    B, H, W, C4 = y.shape
    return y.reshape(B, H, W, C4 // 4, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * H, 2 * W, C4 // 4)


def epilogue_f64(y: torch.Tensor, bias=None, act=None, mul=None, alpha: float = 1.0, res=None, gate_pairs: bool = False,
                 shuffle: int = 0, gelu: str = "erf") -> torch.Tensor:
    """The GEMM epilogue in fp64 on channel-last y: res + alpha * mul * act(y + bias), pixel-shuffled before the residual;
    gate_pairs: (y + bias)[..., 2j] * (y + bias)[..., 2j + 1] and nothing else.  alpha * mul is formed in fp32 as the kernels do."""
    assert y.dtype == torch.float64
    if bias is not None:
        y = y + bias.double()
    if gate_pairs:
        assert act is None and mul is None and res is None and shuffle == 0 and alpha == 1.0
        return y[..., 0::2] * y[..., 1::2]
    y = act_f64(y, act, gelu)
    if mul is not None:
        y = y * (mul.float() * alpha).double()
    elif alpha != 1.0:
        y = y * float(torch.tensor(alpha, dtype=torch.float32))
    if shuffle == 2:
        y = pixel_shuffle2_nhwc(y)
    if res is not None:
        y = y + res.double()
    return y


def layernorm_f64(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float) -> torch.Tensor:
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    var = (xd - mu).pow(2).mean(-1, keepdim=True)
    return (xd - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def chunked_fp32_matmul(a: torch.Tensor, w: torch.Tensor, chunk: int = 16) -> torch.Tensor:
    """a [M, K] @ w [N, K]^T accumulated in fp32, `chunk` k-values per step (the MFMA's depth): the arithmetic the reference stands in for."""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32, device=a.device)
    for k0 in range(0, a.shape[1], chunk):
        acc = acc + a[:, k0:k0 + chunk].float().matmul(w[:, k0:k0 + chunk].float().t())
    return acc


def rel_err(out: torch.Tensor, ref: torch.Tensor) -> float:
    """max|out - ref| / max(1, max|ref|), in fp64."""
    return (out.double() - ref.double()).abs().max().item() / max(1.0, ref.abs().max().item())


def bf16_row_excess(out: torch.Tensor, ref: torch.Tensor, tol: float = FP32_CHAIN_TOL) -> float:
    """Largest |out - ref| - (2^-8 |ref| + tol * max(1, max|ref|)) over the elements: <= 0 when a bf16-stored output is within half a
    bf16 ulp plus the fp32 bound of the reference."""
    ref = ref.double()
    bound = ref.abs() * 2.0 ** -8 + tol * max(1.0, ref.abs().max().item())
    return ((out.double() - ref).abs() - bound).max().item()
