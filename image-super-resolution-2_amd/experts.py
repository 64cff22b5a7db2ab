"""The three frozen experts sequenced on the HIP kernels: HAT-L, DAT, NAFNet-SR.

Each class takes the reference-keyed state dict, prepares device weights once (repacking, BN folding,
position-bias tables) and exposes forward(lr NCHW [1,3,h,w]) -> SR NCHW [1,3,4h,4w] clamped to [0,1]
with the semantics of ExpertEnsemble.forward_hat/_dat/_nafnet (src/models/expert_loader.py:591-674):
reflect-pad to x16, run, crop, clamp.  Activations are NHWC fp32 device tensors; every arithmetic
step is a libff_hip.so kernel (ops.py), PyTorch only allocates.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import ops
from .prep import (pack_conv, pack_dw, bn_scale_shift, fold_bn_after_conv, pack_token_linear, pack_naf_ffn, pack_naf_tail,
                   pack_win_attn, pack_win_rel, pack_token_projmlp, pack_chan_qkv, pack_token_linear_gated, pack_rel_overlap, pack_ocab_qkv)

T = torch.Tensor
SD = Dict[str, T]
RGB_MEAN = (0.4488, 0.4371, 0.4040)


def _ceil_to(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _forward_batch(who: str, name: str, lr: T, taps: Optional[dict], feats: Optional[dict], out: Optional[T], nb_bound, feat_shape, chunk) -> T:
    """The batch driver of the experts' forward(): B == 1 (or a batch that fits one chunk) is one chunk(lr, taps, feats, out, None, B);
    a larger batch runs in chunks of nb images, every chunk writing its slice of the one output (and feature) buffer, feats[name] = the
    feature buffer.  nb_bound(): the expert's images-per-chunk bound in the fused modes (the f32 mode loops per image); feat_shape: the
    hooked feature's shape for the whole batch; chunk(lr, taps, feats, out, feat_out, cap): the expert's _forward_chunk, cap = the
    largest chunk's images."""
    B, _, h, w = lr.shape
    if B > 1:
        if taps is not None:
            raise ops._lib.FFError(f"{who}.forward: taps are recorded for B == 1 only")
        nb = max(1, nb_bound()) if ops.fused_modes() else 1      # images per chunk
        if nb < B:
            if out is None:
                out = torch.empty((B, 3, 4 * h, 4 * w), device=lr.device, dtype=torch.float32)
            fall = ops.empty_rows(feat_shape, lr.device) if feats is not None else None
            for b0 in range(0, B, nb):
                chunk(lr[b0:b0 + nb], None, {} if feats is not None else None, out[b0:b0 + nb],
                      fall[b0:b0 + nb] if feats is not None else None, nb)
            if feats is not None:
                feats[name] = fall
            return out
    return chunk(lr, taps, feats, out, None, B)


class _Weights:
    """Small helper: fetch tensors by reference key, move to the device once."""

    def __init__(self, sd: SD, dev, prefix: str):
        self.sd, self.dev, self.p = sd, dev, prefix

    def __call__(self, name: str) -> T:
        return self.sd[self.p + name].to(self.dev, torch.float32).contiguous()

    def conv(self, name: str) -> T:
        return pack_conv(self(name + ".weight"))

    def opt(self, name: str) -> Optional[T]:
        k = self.p + name
        return self.sd[k].to(self.dev, torch.float32).contiguous() if k in self.sd else None


def _packed(blk: dict, key: str, build):
    """blk[key], made by build() on first use: the repacked weights only one contraction mode's kernels read are prepared lazily,
    once, and kept beside the tensors they were made from (the key is the slot name a recorded plan stores: plan.py)."""
    pk = blk.get(key)
    if pk is None:
        pk = blk[key] = build()
    return pk


def _tl(blk: dict, key: str) -> dict:
    """ff_token_linear weights of blk[key] = (W [N,K], b)."""
    return _packed(blk, key + "_tl", lambda: pack_token_linear(*blk[key]))


def _pm(blk: dict) -> dict:
    return _packed(blk, "projmlp_pk", lambda: pack_token_projmlp(*blk["proj"], *blk["fc1"], *blk["fc2"]))


def _wf(blk: dict, heads: int, d: int) -> dict:
    """ff_win_attn_fused weights of blk["qkv"] = (W [3C, C], b)."""
    return _packed(blk, "qkv_wf", lambda: pack_win_attn(*blk["qkv"], heads, d, d ** -0.5))


class _Trunk:
    """What HAT and DAT share around their residual groups (hat_arch.py:905-984, dat_arch.py:940-1028): conv_first on the mean-shifted,
    reflect-padded input, and after the groups the final LayerNorm, conv_after_body with the long residual, the x4 pixel-shuffle
    tail and conv_last with "+ mean" folded into its bias.  `name` is the key of the hooked feature."""

    def _load_trunk(self, w: _Weights, dev) -> None:
        self.neg_mean = torch.tensor([-m for m in RGB_MEAN], device=dev)
        self.conv_first = (w.conv("conv_first"), w("conv_first.bias"))
        self.norm = (w("norm.weight"), w("norm.bias"))
        self.after = (w.conv("conv_after_body"), w("conv_after_body.bias"))
        self.before_up = (w.conv("conv_before_upsample.0"), w("conv_before_upsample.0.bias"))
        self.up0 = (w.conv("upsample.0"), w("upsample.0.bias"))
        self.up2 = (w.conv("upsample.2"), w("upsample.2.bias"))
        self.last = (w.conv("conv_last"), (w("conv_last.bias") - self.neg_mean).contiguous())   # "+ mean" folded into the bias

    def _enter(self, lr: T, Hp: int, Wp: int) -> T:
        """lr [B,3,h,w] -> conv_first's output [B,Hp,Wp,180].  per_image matters for B > 1 only (ops.conv2d), here and in _exit."""
        xin = ops.nchw_to_nhwc(lr, Hp, Wp, add=self.neg_mean, pad_mode="reflect")
        return ops.conv2d(xin, *self.conv_first, ksize=(3, 3), pad=(1, 1), per_image=True)

    def _exit(self, x: T, feat: T, h: int, w: int, feats: Optional[dict], out: Optional[T], feat_out: Optional[T] = None) -> T:
        """The groups' output x and conv_first's feat -> SR [B,3,4h,4w] (into `out` when given).  feats (optional dict): receives
        feats[name] = the conv_after_body output [B,Hp,Wp,180] (NHWC, into `feat_out` when given), the tensor the reference's forward
        hook captures for the cached-expert files (expert_loader.py:838, :850); the residual is then a launch of its own."""
        x = ops.layernorm(x, *self.norm)
        if feats is not None:
            feats[self.name] = ops.conv2d(x, *self.after, ksize=(3, 3), pad=(1, 1), per_image=True, out=feat_out)
            x = ops.mix2(feats[self.name], feat)
        else:
            x = ops.conv2d(x, *self.after, ksize=(3, 3), pad=(1, 1), res=feat, per_image=True)
        x = ops.conv2d(x, *self.before_up, ksize=(3, 3), pad=(1, 1), act="lrelu", per_image=True)
        x = ops.conv2d(x, *self.up0, ksize=(3, 3), pad=(1, 1), shuffle=2, per_image=True)
        x = ops.conv2d(x, *self.up2, ksize=(3, 3), pad=(1, 1), shuffle=2, per_image=True)
        sr = ops.conv2d(x, *self.last, ksize=(3, 3), pad=(1, 1), per_image=True)
        return ops.nhwc_to_nchw(sr, 4 * h, 4 * w, clamp01=True, out=out)


# =============================================================================================== HAT
def _rel_index_sa(ws: int) -> T:
    ys, xs = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    yy, xx = ys.reshape(-1), xs.reshape(-1)
    return (yy[:, None] - yy[None, :] + ws - 1) * (2 * ws - 1) + (xx[:, None] - xx[None, :] + ws - 1)


def _rel_index_oca(ws: int, ows: int) -> T:
    ys, xs = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    ye, xe = torch.meshgrid(torch.arange(ows), torch.arange(ows), indexing="ij")
    dy = ye.reshape(-1)[None, :] - ys.reshape(-1)[:, None] + ws - ows + 1
    dx = xe.reshape(-1)[None, :] - xs.reshape(-1)[:, None] + ws - ows + 1
    return dy * (ws + ows - 1) + dx


class HatHIP(_Trunk):
    """HAT-L (hat_arch.py:710-984): 12 RHAG x (6 HAB + OCAB), dim 180, 6 heads, window 16.

    forward(lr [B,3,h,w]) runs a batch through ONE launch per op in the fused modes: the window, row and 3x3 kernels take B or plain
    row counts, and the only per-image quantity -- the channel-attention gate -- is a [B,180] matrix (per-image pool partials from the
    convolution's epilogue, one finish + MLP workgroup per image, a per-image scale in token_projmlp).  Every choice of kernel route is
    made from ONE image's dimensions, so each image comes out with the bits of its own B == 1 forward."""

    # Batches are processed in chunks of at most this many padded tokens (B * Hp * Wp): four 256 x 256 tiles, i.e. activation memory
    # grows to at most four times what one such tile allocates.  An attribute, not an environment switch.  It bounds HAT alone: in
    # FreqFusionHIP.forward the DAT and NAFNet outputs and the fusion.pre tensors of EVERY image of the batch live until the join, so
    # that part of the memory grows linearly with B (model._run_experts).  forward() also keeps a chunk below the 2^31 input
    # elements up to which ops.conv2d takes the LDS-resident 3x3 kernel, so raising this value cannot move a batch to another route.
    max_batch_tokens = 262144
    name = "hat"

    def __init__(self, sd: SD, dev, prefix: str = "expert_ensemble.hat.", groups: int = 12, depth: int = 6, ws: int = 16,
                 heads: int = 6, conv_scale: float = 0.01):
        w = _Weights(sd, dev, prefix)
        self.dev, self.ws, self.heads, self.groups, self.depth, self.conv_scale = dev, ws, heads, groups, depth, conv_scale
        self.ows = ws + ws // 2
        self._load_trunk(w, dev)
        rpi_sa = _rel_index_sa(ws).reshape(-1).to(dev)
        rpi_oca = _rel_index_oca(ws, self.ows).reshape(-1).to(dev)
        n, nk = ws * ws, self.ows * self.ows

        def lin(name):
            return w(name + ".weight"), w(name + ".bias")

        self.pe_norm = (w("patch_embed.norm.weight"), w("patch_embed.norm.bias"))
        self.blocks: List[List[dict]] = []
        self.ocab: List[dict] = []
        self.gconv = []
        for g in range(groups):
            blks = []
            for b in range(depth):
                q = f"layers.{g}.residual_group.blocks.{b}."
                tbl = w(q + "attn.relative_position_bias_table")
                bias = tbl[rpi_sa].reshape(n, n, heads).permute(2, 1, 0).contiguous()      # [heads][key][query]
                blks.append(dict(rel=tbl.t().contiguous(),                                 # [heads][(2ws-1)^2] compact table
                    n1=(w(q + "norm1.weight"), w(q + "norm1.bias")), qkv=lin(q + "attn.qkv"), proj=lin(q + "attn.proj"),
                    bias=bias, cab0=(w.conv(q + "conv_block.cab.0"), w(q + "conv_block.cab.0.bias")),
                    cab2=(w.conv(q + "conv_block.cab.2"), w(q + "conv_block.cab.2.bias")),
                    ca1=(w(q + "conv_block.cab.3.attention.1.weight").reshape(-1, 180).contiguous(), w(q + "conv_block.cab.3.attention.1.bias")),
                    ca2=(w(q + "conv_block.cab.3.attention.3.weight").reshape(180, -1).contiguous(), w(q + "conv_block.cab.3.attention.3.bias")),
                    n2=(w(q + "norm2.weight"), w(q + "norm2.bias")), fc1=lin(q + "mlp.fc1"), fc2=lin(q + "mlp.fc2"),
                    shift=0 if b % 2 == 0 else ws // 2))
            self.blocks.append(blks)
            q = f"layers.{g}.residual_group.overlap_attn."
            tbl = w(q + "relative_position_bias_table")
            self.ocab.append(dict(
                n1=(w(q + "norm1.weight"), w(q + "norm1.bias")), qkv=lin(q + "qkv"), proj=lin(q + "proj"),
                bias=tbl[rpi_oca].reshape(n, nk, heads).permute(2, 1, 0).contiguous(), rel=pack_rel_overlap(tbl, ws, self.ows),
                n2=(w(q + "norm2.weight"), w(q + "norm2.bias")), fc1=lin(q + "mlp.fc1"), fc2=lin(q + "mlp.fc2")))
            self.gconv.append((w.conv(f"layers.{g}.conv"), w(f"layers.{g}.conv.bias")))

    # -- blocks -------------------------------------------------------------------------------
    def _mlp(self, x: T, blk: dict) -> T:
        """x + MLP(norm2(x)) of the f32 route; the fused modes run it inside token_projmlp."""
        xn = ops.layernorm(x, *blk["n2"])
        h = ops.linear(xn, *blk["fc1"], act="gelu")
        return ops.linear(h, *blk["fc2"], res=x)

    def hab(self, x: T, blk: dict) -> T:
        _, H, W, C = x.shape
        d = C // self.heads
        fused = ops.fused_modes()
        # plain bf16: att, the normalised rows and conv1's output are consumed only as MFMA operands (rounded to bf16 there), so they are
        # stored as bf16 -- bit-identical results, half the bytes; conv2's output enters x1 times conv_scale = 0.01 and goes the same way
        b16 = ops.gemm_mode() == "bf16" and H * W >= 1024 and C % 4 == 0     # (one image's pixels: the route must not depend on B)
        att = ops.empty_rows_bf16(tuple(x.shape), x.device) if b16 else ops.empty_like_rows(x)
        s = blk["shift"]
        if fused:                                                  # norm1 + qkv + (S)W-MSA of all six heads in one launch (csrc/win_attn_fused.hip)
            relp = _packed(blk, "relp", lambda: pack_win_rel(blk["rel"], self.ws, self.ws))
            _, xn = ops.win_attn_fused(x, att, _wf(blk, self.heads, d), relp, gamma=blk["n1"][0], beta=blk["n1"][1], H=H, W=W,
                                       Hp=H, Wp=W, win=(self.ws, self.ws), shift=(s, s), use_mask=s > 0, want_xn="bf16" if b16 else True)
        else:
            xn = ops.layernorm(x, *blk["n1"])
            qkv = ops.linear(xn, *blk["qkv"])
            # the bias streams from the expanded quad-interleaved table: gathering it from the compact relative-position table in LDS
            # removes the 400 MB / launch bias stream but measured SLOWER on MI355X (120 vs 108 us per launch: the kernel is issue /
            # LDS bound, not bandwidth bound)
            ops.window_attn(qkv, att, blk["bias"], q_off=0, k_off=C, v_off=2 * C, o_off=0, H=H, W=W, Hp=H, Wp=W, win=(self.ws, self.ws),
                            kwin=(self.ws, self.ws), shift=(s, s), use_mask=s > 0, heads=self.heads, d=d, scale=d ** -0.5)
        if b16 and self._cab_fused(xn):                            # both convolutions in one launch, c1 in LDS (csrc/cab_fused.hip): same bits
            c2, c2mean = ops.cab_fused(xn, blk["cab0"], blk["cab2"])
        else:
            c1 = ops.conv2d(xn, *blk["cab0"], ksize=(3, 3), pad=(1, 1), act="gelu", out_bf16=b16, per_image=True)
            c2, c2mean = ops.conv2d(c1, *blk["cab2"], ksize=(3, 3), pad=(1, 1), want_pool="partials", out_bf16=b16)   # pool partials from the conv epilogue
        gate = ops.vec_mlp(c2mean, *blk["ca1"], "relu", *blk["ca2"], "sigmoid", post=self.conv_scale)
        if fused:                                                  # proj + both residuals + norm2 + MLP: x1 never reaches memory
            # gate [B,180]: one launch for the batch, image b scaled by its own row
            return ops.token_projmlp(att, x, _pm(blk), blk["n2"][0], blk["n2"][1], c2=c2, c2_scale=gate if x.shape[0] > 1 else gate.reshape(-1))
        t = ops.mix2(x, c2, cb=gate)
        x = ops.linear(att, *blk["proj"], res=t)
        return self._mlp(x, blk)

    def ocab_block(self, x: T, blk: dict) -> T:
        _, H, W, C = x.shape
        d = C // self.heads
        fused = ops.fused_modes()
        rows16 = ops.gemm_mode() == "bf16" and (self.ws, self.ows, d) == (16, 24, 30) and H % 16 == 0 and W % 16 == 0
        if rows16:
            # q / k / v have one consumer, the attention kernel, which rounds them to bf16 (q after the scale): the projection writes
            # exactly those roundings as head-padded bf16 rows (30 -> 32 channels: 64-byte, 16-byte aligned head slices)
            pk = _packed(blk, "qkv_r16", lambda: pack_ocab_qkv(*blk["qkv"], self.heads, d))
            qkv = ops.token_linear_rows16(x, pk, gamma=blk["n1"][0], beta=blk["n1"][1])            # LayerNorm fused
        elif fused:
            qkv = ops.token_linear(x, _tl(blk, "qkv"), gamma=blk["n1"][0], beta=blk["n1"][1])      # LayerNorm fused
        else:
            qkv = ops.linear(ops.layernorm(x, *blk["n1"]), *blk["qkv"])
        if rows16:
            att = ops.empty_rows_bf16(tuple(x.shape), x.device)    # consumed only as an MFMA operand, as in hab
            hp = self.heads * 32
            ops.ocab_attn_rows16(qkv, att, blk["rel"], q_off=0, k_off=hp, v_off=2 * hp, H=H, W=W, heads=self.heads, d=d, ws=self.ws,
                                 ows=self.ows)             # persistent per-window kernel, compact bias table in LDS (csrc/ocab_attn.hip)
        else:
            # 576 keys per window, the bias streams from the expanded table (3.5 MB per head): gathering it in window_attn from the
            # rotated compact table in LDS is bit-identical and 430 MB less traffic per launch, but 314 vs 207 us on MI355X (two
            # dependent LDS reads per score)
            att = ops.empty_like_rows(x)
            ops.window_attn(qkv, att, blk["bias"], q_off=0, k_off=C, v_off=2 * C, o_off=0, H=H, W=W, Hp=H, Wp=W, win=(self.ws, self.ws),
                            kwin=(self.ows, self.ows), shift=(0, 0), use_mask=False, heads=self.heads, d=d, scale=d ** -0.5)
        if fused:
            return ops.token_projmlp(att, x, _pm(blk), blk["n2"][0], blk["n2"][1])
        x = ops.linear(att, *blk["proj"], res=x)
        return self._mlp(x, blk)

    def _cab_fused(self, xn: T) -> bool:
        """True where CAB's two convolutions run as one launch (ops.cab_fused): plain bf16 on hab()'s b16 route, 180 channels, H and W
        multiples of 16.  Bit-equal to the two launches, so the route may differ between shapes without moving a result."""
        return ops.cab_fused_ok(xn)

    def _linked(self, x: T) -> bool:
        """True where a group's HABs run as attention, (CAB, hab_link) x 5, CAB, token_projmlp: plain bf16 on hab()'s b16 route, at the
        shape csrc/hab_link.hip is built for.  (The row-offset bound counts the batch; the link is bit-equal to the pair of launches
        it replaces, so an image still comes out with the bits of its own B == 1 forward.)"""
        B, H, W, C = x.shape
        return (ops.gemm_mode() == "bf16" and H * W >= 1024 and (self.ws, self.heads, C) == (16, 6, 180) and H % 16 == 0 and W % 16 == 0
                and B * H * W * 192 < 2 ** 31)

    def _habs_linked(self, x: T, blks: List[dict]) -> T:
        """hab() over blks with every block's token_projmlp and the next block's win_attn_fused in one launch (ops.hab_link): the next
        attention takes x from the MLP's accumulators instead of reading it back.  Same values as the hab() loop, bit for bit."""
        B, H, W, C = x.shape
        d, win = C // self.heads, (self.ws, self.ws)

        def relp(blk):
            return _packed(blk, "relp", lambda: pack_win_rel(blk["rel"], self.ws, self.ws))

        s = blks[0]["shift"]
        att = ops.empty_rows_bf16(tuple(x.shape), x.device)
        _, xn = ops.win_attn_fused(x, att, _wf(blks[0], self.heads, d), relp(blks[0]), gamma=blks[0]["n1"][0], beta=blks[0]["n1"][1], H=H, W=W,
                                   Hp=H, Wp=W, win=win, shift=(s, s), use_mask=s > 0, want_xn="bf16")
        for i, blk in enumerate(blks):
            if self._cab_fused(xn):
                c2, c2mean = ops.cab_fused(xn, blk["cab0"], blk["cab2"])
            else:
                c1 = ops.conv2d(xn, *blk["cab0"], ksize=(3, 3), pad=(1, 1), act="gelu", out_bf16=True, per_image=True)
                c2, c2mean = ops.conv2d(c1, *blk["cab2"], ksize=(3, 3), pad=(1, 1), want_pool="partials", out_bf16=True)
            gate = ops.vec_mlp(c2mean, *blk["ca1"], "relu", *blk["ca2"], "sigmoid", post=self.conv_scale)
            gate = gate if B > 1 else gate.reshape(-1)
            if i + 1 < len(blks):
                nxt = blks[i + 1]
                s = nxt["shift"]
                x, xn, att = ops.hab_link(att, x, _pm(blk), blk["n2"][0], blk["n2"][1], c2=c2, c2_scale=gate, wf=_wf(nxt, self.heads, d),
                                          rel_padded=relp(nxt), gamma1=nxt["n1"][0], beta1=nxt["n1"][1], shift=(s, s), use_mask=s > 0)
            else:
                x = ops.token_projmlp(att, x, _pm(blk), blk["n2"][0], blk["n2"][1], c2=c2, c2_scale=gate)
        return x

    def group(self, x: T, g: int) -> T:
        if self._linked(x):
            y = self._habs_linked(x, self.blocks[g])
        else:
            y = x
            for blk in self.blocks[g]:
                y = self.hab(y, blk)
        y = self.ocab_block(y, self.ocab[g])
        return ops.conv2d(y, *self.gconv[g], ksize=(3, 3), pad=(1, 1), res=x, per_image=True)

    def forward(self, lr: T, taps: Optional[dict] = None, feats: Optional[dict] = None, out: Optional[T] = None) -> T:
        """lr [B,3,h,w] -> [B,3,4h,4w] (written into `out` when given).  feats (optional dict): receives feats["hat"] (_Trunk._exit).
        B > 1: one launch per op for the whole batch in the fused modes (chunks of max_batch_tokens padded tokens), the per-image
        loop in f32 mode; either way bit-equal to B single forwards.  taps are recorded for B == 1 only."""
        B, _, h, w = lr.shape
        Hp, Wp = _ceil_to(h, self.ws), _ceil_to(w, self.ws)
        # ops.conv2d keeps the LDS-resident 3x3 kernel to inputs of fewer than 2^31 elements (32-bit offsets), counted over the whole
        # launch.  The largest 3x3 input here is the last convolution's, 16 Hp Wp pixels at a pitch of 64: a chunk stays under that
        # bound whatever max_batch_tokens says, so a batch never leaves the route its images take alone.
        return _forward_batch("HatHIP", "hat", lr, taps, feats, out,
                              lambda: min(int(self.max_batch_tokens) // (Hp * Wp), (2 ** 31 - 1) // (16 * Hp * Wp * 64)),
                              (B, Hp, Wp, self.after[0].shape[0]),
                              lambda x, tp, ft, o, fo, cap: self._forward_chunk(x, tp, ft, o, fo))

    def _forward_chunk(self, lr: T, taps: Optional[dict], feats: Optional[dict], out: Optional[T], feat_out: Optional[T]) -> T:
        """One launch per op for all of lr [B,3,h,w]; feat_out: where the hooked feature goes (a slice of the batch's buffer)."""
        _, _, h, w = lr.shape
        Hp, Wp = _ceil_to(h, self.ws), _ceil_to(w, self.ws)
        feat = self._enter(lr, Hp, Wp)
        x = ops.layernorm(feat, *self.pe_norm)
        for g in range(self.groups):
            if taps is not None and g == 0:
                y = x
                for b, blk in enumerate(self.blocks[0]):
                    y = self.hab(y, blk)
                    taps[f"hat.g0.b{b}"] = y
                y = self.ocab_block(y, self.ocab[0])
                taps["hat.g0.ocab"] = y
                x = ops.conv2d(y, *self.gconv[0], ksize=(3, 3), pad=(1, 1), res=x)       # (taps: B == 1)
                taps["hat.g0.out"] = x
            else:
                x = self.group(x, g)
        return self._exit(x, feat, h, w, feats, out, feat_out)


# =============================================================================================== DAT
def _dat_dpb_bias(sd: SD, p: str, hs: int, wsz: int, heads: int) -> T:
    """DynamicPosBias (dat_arch.py:177-212) is input independent: evaluate it once on the host."""
    import torch.nn.functional as F
    ys, xs = torch.meshgrid(torch.arange(1 - hs, hs), torch.arange(1 - wsz, wsz), indexing="ij")
    t = F.linear(torch.stack([ys.reshape(-1), xs.reshape(-1)], dim=1).float(), sd[p + ".pos_proj.weight"].float().cpu(),
                 sd[p + ".pos_proj.bias"].float().cpu())
    for j in ("pos1", "pos2", "pos3"):
        t = F.layer_norm(t, (t.shape[-1],), sd[f"{p}.{j}.0.weight"].float().cpu(), sd[f"{p}.{j}.0.bias"].float().cpu())
        t = F.linear(F.relu(t), sd[f"{p}.{j}.2.weight"].float().cpu(), sd[f"{p}.{j}.2.bias"].float().cpu())
    cy, cx = torch.meshgrid(torch.arange(hs), torch.arange(wsz), indexing="ij")
    cy, cx = cy.reshape(-1), cx.reshape(-1)
    idx = (cy[:, None] - cy[None, :] + hs - 1) * (2 * wsz - 1) + (cx[:, None] - cx[None, :] + wsz - 1)
    n = hs * wsz
    # expanded [heads][key][query] for the f32 kernel, compact [heads][(2hs-1)*(2wsz-1)] for the LDS gather of the bf16 kernel
    return t[idx.reshape(-1)].reshape(n, n, heads).permute(2, 1, 0).contiguous(), t.t().contiguous()


def dat_should_shift(g: int, b: int) -> bool:
    return (g % 2 == 0 and b > 0 and (b - 2) % 4 == 0) or (g % 2 != 0 and b % 4 == 0)


class DatHIP(_Trunk):
    """DAT (dat_arch.py:864-1028): 6 residual groups x 6 DATB (spatial / channel alternating), dim 180.

    forward(lr [B,3,h,w]) runs a batch through ONE launch per op in the fused modes.  DAT pads to multiples of 16, so an image is a
    multiple of 256 token rows and neither a 256-token workgroup nor a GEMM tile straddles two images.  The per-image quantities are the
    channel blocks' attention matrix wbd [B,180,180] (per-image reduction of the gram partials, per-image weight planes in the att GEMM)
    and the channel gate cm [B,180] (per-image pool partials, one MLP workgroup per image, a per-image row in token_linear_gated); the
    window, depth-wise, SGFN and 3x3 kernels index the image themselves.  Every choice of kernel route is made from ONE image's
    dimensions, so each image comes out with the bits of its own B == 1 forward."""

    # Batches are processed in chunks of at most this many padded tokens (B * Hp * Wp), as HatHIP does: activation memory grows to at most
    # four times what one 256 x 256 tile allocates.  An attribute, not an environment switch.  forward() also keeps a chunk below the
    # 32-bit bounds of what it launches, whatever this value says (see there).
    max_batch_tokens = 262144
    name = "dat"

    def __init__(self, sd: SD, dev, prefix: str = "expert_ensemble.dat.", groups: int = 6, depth: int = 6, split=(8, 32),
                 heads: int = 6):
        w = _Weights(sd, dev, prefix)
        self.dev, self.groups, self.depth, self.split, self.heads = dev, groups, depth, split, heads
        self._load_trunk(w, dev)
        C = 180

        def lin(name):
            return w(name + ".weight"), w(name + ".bias")

        def folded_1x1(conv, bn, cin):
            wt = w(conv + ".weight").reshape(-1, cin)
            sc, sh = bn_scale_shift({k: v.to(dev) for k, v in sd.items() if k.startswith(prefix + bn)}, prefix + bn)
            return fold_bn_after_conv(wt, w(conv + ".bias"), sc, sh)

        self.before = (w("before_RG.1.weight"), w("before_RG.1.bias"))
        self.blocks: List[List[dict]] = []
        self.gconv = []
        for g in range(groups):
            blks = []
            for b in range(depth):
                q = f"layers.{g}.blocks.{b}."
                sc, sh = bn_scale_shift({k: v.to(dev) for k, v in sd.items() if k.startswith(prefix + q + "attn.dwconv.1")},
                                        prefix + q + "attn.dwconv.1")
                ci1 = folded_1x1(q + "attn.channel_interaction.1", q + "attn.channel_interaction.2", C)
                si0 = folded_1x1(q + "attn.spatial_interaction.0", q + "attn.spatial_interaction.1", C)
                blk = dict(
                    spatial=(b % 2 == 0), shifted=dat_should_shift(g, b),
                    n1=(w(q + "norm1.weight"), w(q + "norm1.bias")), qkv=lin(q + "attn.qkv"), proj=lin(q + "attn.proj"),
                    dw=(pack_dw(w(q + "attn.dwconv.0.weight")), w(q + "attn.dwconv.0.bias"), sc, sh),
                    ci1=ci1, ci4=(w(q + "attn.channel_interaction.4.weight").reshape(C, -1).contiguous(), w(q + "attn.channel_interaction.4.bias")),
                    si0=si0, si3=(w(q + "attn.spatial_interaction.3.weight").reshape(1, -1).contiguous(), w(q + "attn.spatial_interaction.3.bias")),
                    n2=(w(q + "norm2.weight"), w(q + "norm2.bias")), fc1=lin(q + "ffn.fc1"),
                    sgn=(w(q + "ffn.sg.norm.weight"), w(q + "ffn.sg.norm.bias")),
                    sgc=(pack_dw(w(q + "ffn.sg.conv.weight")), w(q + "ffn.sg.conv.bias")), fc2=lin(q + "ffn.fc2"))
                if blk["spatial"]:
                    pb = [_dat_dpb_bias(sd, prefix + q + "attn.attns.0.pos", split[0], split[1], heads // 2),
                          _dat_dpb_bias(sd, prefix + q + "attn.attns.1.pos", split[1], split[0], heads // 2)]
                    blk["bias"] = [pb[0][0].to(dev), pb[1][0].to(dev)]
                    blk["rel"] = [pb[0][1].to(dev), pb[1][1].to(dev)]
                else:
                    blk["temp"] = w(q + "attn.temperature").reshape(-1).contiguous()
                blk["si3b"] = float(blk["si3"][1].reshape(-1)[0].cpu())                    # scalar bias of the 11 -> 1 layer
                blks.append(blk)
            self.blocks.append(blks)
            self.gconv.append((w.conv(f"layers.{g}.conv"), w(f"layers.{g}.conv.bias")))

    def block(self, x: T, blk: dict) -> T:
        B, H, W, C = x.shape
        half, hh = C // 2, self.heads // 2
        d = half // hh
        fused = ops.fused_modes()
        if blk["spatial"]:
            m = max(self.split)
            Hp, Wp = _ceil_to(H, m), _ceil_to(W, m)
        if fused and blk["spatial"]:
            # norm1 + qkv + both window-attention branches: two launches (head groups 0-2 on 8x32 windows, 3-5 on 32x8), each
            # also writes its half of v for the depth-wise conv branch (dat_arch.py:524); q and k never reach memory
            att = ops.empty_like_rows(x)
            v = ops.empty_like_rows(x)
            pk = _wf(blk, self.heads, d)

            def rel6(br, wh, ww):                                  # the branch's bias table in its three rows of six, the others zero
                r6 = torch.zeros(self.heads, blk["rel"][br].shape[1], device=x.device)
                r6[hh * br:hh * br + hh] = blk["rel"][br]
                return pack_win_rel(r6, wh, ww)
            relp = _packed(blk, "relp", lambda: [rel6(0, *self.split), rel6(1, *self.split[::-1])])
            for br in range(2):
                wh, ww = (self.split[0], self.split[1]) if br == 0 else (self.split[1], self.split[0])
                sh = (wh // 2, ww // 2) if blk["shifted"] else (0, 0)
                ops.win_attn_fused(x, att, pk, relp[br], gamma=blk["n1"][0], beta=blk["n1"][1], H=H, W=W, Hp=Hp, Wp=Wp,
                                   win=(wh, ww), shift=sh, use_mask=blk["shifted"], head0=hh * br, nheads=hh, zero_pad=True,
                                   v_out=v, v_off=0)
        elif fused:
            # norm1 + qkv + per-head gram / norms over all tokens in one launch: only v reaches memory (dat_arch.py:617-641)
            cq = _packed(blk, "cq_pk", lambda: pack_chan_qkv(*blk["qkv"], self.heads, C // self.heads))
            v, wbd = ops.chan_qkv_attn(x, cq, blk["n1"][0], blk["n1"][1], blk["temp"])      # B > 1: wbd [B,180,180], one matrix per image
        else:
            qkv = ops.linear(ops.layernorm(x, *blk["n1"]), *blk["qkv"])              # [1,H,W,3C] = q | k | v
            v = qkv[..., 2 * C:]
        conv_x = ops.dwconv2d(v, blk["dw"][0], blk["dw"][1], post_scale=blk["dw"][2], post_shift=blk["dw"][3], act="gelu")
        if blk["spatial"]:
            if not fused:
                att = ops.empty_like_rows(x)
                for br in range(2):
                    wh, ww = (self.split[0], self.split[1]) if br == 0 else (self.split[1], self.split[0])
                    sh = (wh // 2, ww // 2) if blk["shifted"] else (0, 0)
                    ops.window_attn(qkv, att, blk["bias"][br], q_off=br * half, k_off=C + br * half, v_off=2 * C + br * half,
                                    o_off=br * half, H=H, W=W, Hp=Hp, Wp=Wp, win=(wh, ww), kwin=(wh, ww), shift=sh,
                                    use_mask=blk["shifted"], heads=hh, d=d, scale=d ** -0.5)
            ch_in, sp_in = conv_x, att
        else:
            if not fused:
                wbd = ops.chan_attn_weights(qkv, 0, C, blk["temp"])
            att = ops.linear(v, wbd, dynamic_w=True)                                 # (B > 1: image b's rows times wbd[b], one launch)
            ch_in, sp_in = att, conv_x
        cm = ops.vec_mlp(ops.pool_partials(ch_in), *blk["ci1"], "gelu", *blk["ci4"], "sigmoid")          # [B,C]; pool finish inside the MLP launch
        if fused:
            # spatial gate (from sp_in, applied to ch_in) + channel gate (applied to sp_in) + projection + residual in one launch
            gp = _packed(blk, "gp_pk", lambda: pack_token_linear_gated(*blk["proj"], *blk["si0"], blk["si3"][0]))
            # cm [B,180]: one launch for the batch, image b gated by its own row
            x = ops.token_linear_gated(sp_in, ch_in, gp, cm if B > 1 else cm.reshape(-1), blk["si3b"], res=x)
            return self._sgfn(x, blk)
        sm = ops.linear(ops.linear(sp_in, *blk["si0"], act="gelu"), *blk["si3"], act="sigmoid")          # [1,H,W,1]
        if blk["spatial"]:
            mixed = ops.mix2(att, conv_x, ca=cm, pb=sm)
        else:
            mixed = ops.mix2(att, conv_x, pa=sm, cb=cm)
        x = ops.linear(mixed, *blk["proj"], res=x)
        return self._sgfn(x, blk)

    def _sgfn(self, x: T, blk: dict) -> T:
        """x + SGFN(norm2(x)) (dat_arch.py:155-170, :736)."""
        if ops.fused_modes():
            # fc1 + GELU also emits the SpatialGate LayerNorm statistics of its upper half; the depth-wise conv normalises on load:
            # 101 us against 45 + 72 us for a separate LayerNorm pass + the plain strip kernel (tools/block_timeline.py)
            c2 = blk["fc1"][0].shape[0] // 2
            y, stats = ops.token_linear(x, _tl(blk, "fc1"), gamma=blk["n2"][0], beta=blk["n2"][1], act="gelu", stats_range=(c2, 2 * c2))
            if ops.gemm_mode() == "bf16" and blk["fc2"][0].shape[0] <= 192 and c2 % 4 == 0 and c2 <= 512:
                # SpatialGate + fc2 + residual in one launch: the gate product never reaches memory (csrc/sgfn_tail.hip)
                return ops.sgfn_tail(y, c2, blk["sgc"][0], blk["sgc"][1], stats, blk["sgn"][0], blk["sgn"][1], blk["fc2"][0], blk["fc2"][1], res=x)
            z = ops.dwconv3x3_ln(y[..., c2:], blk["sgc"][0], blk["sgc"][1], stats, blk["sgn"][0], blk["sgn"][1], mul_in=y[..., :c2])
            return ops.linear(z, *blk["fc2"], res=x)
        y = ops.linear(ops.layernorm(x, *blk["n2"]), *blk["fc1"], act="gelu")
        c2 = y.shape[-1] // 2
        gte = ops.layernorm(y[..., c2:], *blk["sgn"])
        z = ops.dwconv2d(gte, *blk["sgc"], mul_in=y[..., :c2])                     # dw3x3(LN(x2)) * x1 in one pass
        return ops.linear(z, *blk["fc2"], res=x)

    def forward(self, lr: T, taps: Optional[dict] = None, feats: Optional[dict] = None, out: Optional[T] = None) -> T:
        """lr [B,3,h,w] -> [B,3,4h,4w] (written into `out` when given).  feats (optional dict): receives feats["dat"] (_Trunk._exit).
        B > 1: one launch per op for the whole batch in the fused modes (chunks of max_batch_tokens padded tokens), the per-image
        loop in f32 mode (its channel attention and dynamic-weight GEMM are single-image); either way bit-equal to B single forwards.
        taps are recorded for B == 1 only."""
        B, _, h, w = lr.shape
        Hp, Wp = _ceil_to(h, 16), _ceil_to(w, 16)

        def nb_bound():
            # Two launches index the whole chunk in 32 bits: the LDS-resident 3x3 kernel (ops.conv2d keeps it to inputs of fewer than
            # 2^31 elements; the largest is the last convolution's, 16 Hp Wp pixels at a pitch of 64) and ff_sgfn_tail (B H W rows of
            # fc1's output at its pitch).  A chunk stays under both whatever max_batch_tokens says, so a batch never leaves the route
            # its images take alone.
            ldh = _ceil_to(self.blocks[0][0]["fc1"][0].shape[0], 32)
            return min(int(self.max_batch_tokens) // (Hp * Wp), (2 ** 31 - 1) // (16 * Hp * Wp * 64), (2 ** 31 - 1) // (Hp * Wp * ldh))
        return _forward_batch("DatHIP", "dat", lr, taps, feats, out, nb_bound, (B, Hp, Wp, self.after[0].shape[0]),
                              lambda x, tp, ft, o, fo, cap: self._forward_chunk(x, tp, ft, o, fo))

    def _forward_chunk(self, lr: T, taps: Optional[dict], feats: Optional[dict], out: Optional[T], feat_out: Optional[T]) -> T:
        """One launch per op for all of lr [B,3,h,w]; feat_out: where the hooked feature goes (a slice of the batch's buffer)."""
        _, _, h, w = lr.shape
        Hp, Wp = _ceil_to(h, 16), _ceil_to(w, 16)
        feat = self._enter(lr, Hp, Wp)
        x = ops.layernorm(feat, *self.before)
        for g in range(self.groups):
            y = x
            for b, blk in enumerate(self.blocks[g]):
                y = self.block(y, blk)
                if taps is not None and g < 2:
                    taps[f"dat.g{g}.b{b}"] = y
            x = ops.conv2d(y, *self.gconv[g], ksize=(3, 3), pad=(1, 1), res=x, per_image=True)
        return self._exit(x, feat, h, w, feats, out, feat_out)


# =============================================================================================== NAFNet-SR
class NafnetHIP:
    """NAFNetSR (nafnet/__init__.py:117-139 + nafnet_arch.py:137-225): bicubic x4, then the width-64
    UNet (enc 2/2/4/8, mid 12, dec 2/2/2/2) at HR resolution.

    forward(lr [B,3,h,w]) runs a batch through ONE launch per op in the fused modes.  The block's only per-image quantities are the SCA
    pool [B,c] and the channel-attention vector it yields (sca / kmul [B,c]); the front, depth-wise and tail kernels and the two conv3
    GEMMs have per-image forms, everything else works on rows.  Every choice of kernel route or tile is made from ONE image's
    dimensions, so each image comes out with the bits of its own B == 1 forward."""

    # Batches are processed in chunks of at most this many padded HR pixels (B * Hp * Wp): four 256 x 256 LR tiles' worth, i.e.
    # activation memory grows to at most four times what one such tile allocates.  An attribute, not an environment switch.
    # forward() also keeps a chunk below the 32-bit bounds of the kernels it launches, whatever this value says: ops.conv2d takes the
    # LDS-resident 3x3 kernel (the ending convolution, 64 channels at HR) for inputs of fewer than 2^31 elements counted over the
    # launch, and ff_naf_tail_images, the two kmul-images GEMMs and the implicit GEMM index rows in 32 bits (B * Hp * Wp < 2^31).
    # B * Hp * Wp * 64 < 2^31 implies all of them, so a batch never leaves the route its images take alone.
    max_batch_pixels = 4 * 1024 * 1024

    def __init__(self, sd: SD, dev, prefix: str = "expert_ensemble.nafnet.nafnet.", enc=(2, 2, 4, 8), mid: int = 12,
                 dec=(2, 2, 2, 2)):
        w = _Weights(sd, dev, prefix)
        self.dev, self.enc_n, self.mid_n, self.dec_n = dev, enc, mid, dec

        def blk(q):
            def c1(n):
                wt = w(q + n + ".weight")
                return wt.reshape(wt.shape[0], wt.shape[1]).contiguous(), w(q + n + ".bias")
            return dict(n1=(w(q + "norm1.weight"), w(q + "norm1.bias")), n2=(w(q + "norm2.weight"), w(q + "norm2.bias")),
                        c1=c1("conv1"), c2=(pack_dw(w(q + "conv2.weight")), w(q + "conv2.bias")), c3=c1("conv3"),
                        sca=c1("sca.1"), c4=c1("conv4"), c5=c1("conv5"),
                        beta=w(q + "beta").reshape(-1).contiguous(), gamma=w(q + "gamma").reshape(-1).contiguous())

        self.intro = (w.conv("intro"), w("intro.bias"))
        self.ending = (w.conv("ending"), w("ending.bias"))
        self.encs = [[blk(f"encoders.{l}.{b}.") for b in range(n)] for l, n in enumerate(enc)]
        self.mids = [blk(f"middle_blks.{b}.") for b in range(mid)]
        self.decs = [[blk(f"decoders.{l}.{b}.") for b in range(n)] for l, n in enumerate(dec)]
        self.downs = [(w.conv(f"downs.{l}"), w(f"downs.{l}.bias")) for l in range(len(enc))]
        self.ups = [w(f"ups.{l}.0.weight").reshape(w(f"ups.{l}.0.weight").shape[0], -1).contiguous() for l in range(len(dec))]

    def _padded_input(self, B: int, Hp: int, Wp: int, dev, cap: Optional[int] = None) -> T:
        """[B,Hp,Wp,3] buffer whose padding (check_image_size, nafnet_arch.py:220-225: zeros right/bottom) was zeroed ONCE when
        the buffer was made; the resampler only ever writes the top-left H x W region, so no fill runs per forward.  Owned by the
        graph entry being captured (its address is in the captured launches) or, for eager forwards, one buffer that is replaced
        when the size changes (ops.persistent_zeros).  cap: the images of the largest chunk of this forward -- the buffer is made
        for cap images and a smaller (remainder) chunk gets its leading slice, so a chunk and its remainder never alternate two
        sizes (which would replace and re-zero the eager buffer every forward)."""
        buf = ops.persistent_zeros(id(self), "naf_in", (max(B, cap or B), Hp, Wp, 3), dev)
        return buf[:B]

    def __del__(self):
        try:
            ops.drop_persistent(owner=id(self))
        except Exception:                                   # interpreter shutdown
            pass

    def block(self, x: T, k: dict, out: Optional[T] = None) -> T:
        """One NAFBlock on x [B,H,W,c]; out: where the result goes (a chunk's slice of the batch's feature buffer)."""
        B, c = x.shape[0], x.shape[-1]
        flash = ops.fused_modes() and c in (64, 128)                         # HR levels: the bandwidth-bound ones
        # deep levels in plain bf16: LayerNorm and the SimpleGate epilogue store the bf16 the GEMM would round to, and conv1 / conv4 /
        # conv5 fetch those rows by LDS-DMA (ops.linear on bf16 rows; bit-equal to the fp32-rows route).  conv3 scales its A operand
        # in fp32 (kmul), so its rows stay fp32 and pass through registers in the same kernel.
        rows = not flash and ops.gemm_mode() == "bf16" and ops.rows_gemm() and ops.rows_gemm_ok(c)
        if flash and c == 64:                                                # LayerNorm2d + conv1 + conv2 + SimpleGate + pool sums: one launch (313 vs 381 us at
                                                                             # 1024 x 1024; the 128-channel form fits one workgroup per CU only and ties: 222 vs 217)
            g, pooled = ops.naf_front(x, _tl(k, "c1"), k["n1"][0], k["n1"][1], *k["c2"])
        else:
            if flash:
                t = ops.token_linear(x, _tl(k, "c1"), gamma=k["n1"][0], beta=k["n1"][1], eps=1e-6)    # LayerNorm2d + conv1
            else:
                t = ops.linear(ops.layernorm(x, *k["n1"], eps=1e-6, out_bf16=rows), *k["c1"], tile_hint=self._rows_tile(x, 2 * c, rows))
            g, pooled = ops.dwconv3_gate_pool(t, *k["c2"])                   # conv2 + SimpleGate + SCA pool sums
        sca = ops.vec_mlp(pooled, *k["sca"], None)                           # [B,c]: one launch for the batch, image b scaled by its own row
        sca = sca if B > 1 else sca.reshape(-1)
        if flash and ops.gemm_mode() == "bf16":                              # plain bf16: conv3 + the gated FFN in one launch, y stays on chip
            tail = _packed(k, "tail_pk", lambda: pack_naf_tail(*k["c3"], *k["c4"], *k["c5"]))
            return ops.naf_tail(g, x, tail, sca, k["beta"], k["n2"][0], k["n2"][1], k["gamma"], out=out)
        nf = ops.gemm_mode() != "f32"                                        # the split-bf16 GEMM carries both NAFBlock fusions
        if nf:                                                               # conv3(g * sca): the scale rides on the A operand
            y = ops.linear(g, *k["c3"], res=x, mul=k["beta"], kmul=sca, rows_gemm=rows)    # (kmul [B,c]: the tile of one image's rows)
        else:
            w3 = ops.mix2(k["c3"][0], ca=sca)                                # conv3(g * sca) == (W3 . diag(sca)) g; f32 mode: B == 1
            y = ops.linear(g, w3, k["c3"][1], res=x, mul=k["beta"], dynamic_w=True)
        if flash:
            ffn = _packed(k, "ffn_pk", lambda: pack_naf_ffn(*k["c4"], *k["c5"]))
            return ops.naf_ffn(y, ffn, k["n2"][0], k["n2"][1], k["gamma"], out=out)
        if nf:                                                               # conv4 + SimpleGate in one launch: the 2c-wide tensor stays on chip
            w4, b4 = k["c4"]                                                 # rows interleaved: 2j <- j, 2j+1 <- j + c (chunk(2, dim=1) halves)
            c4i = _packed(k, "c4i", lambda: (torch.stack((w4[:c], w4[c:]), dim=1).reshape(2 * c, -1).contiguous(),
                                             torch.stack((b4[:c], b4[c:]), dim=1).reshape(-1).contiguous()))
            g = ops.linear(ops.layernorm(y, *k["n2"], eps=1e-6, out_bf16=rows), *c4i, gate_pairs=True, out_bf16=rows,
                           tile_hint=self._rows_tile(y, 2 * c, rows))
        else:
            t = ops.linear(ops.layernorm(y, *k["n2"], eps=1e-6), *k["c4"])
            g = ops.fma3(None, t[..., :c], t[..., c:])
        return ops.linear(g, *k["c5"], res=y, mul=k["gamma"], tile_hint=self._rows_tile(y, c, rows), out=out)

    @staticmethod
    def _rows_tile(x: T, N: int, rows: bool) -> int:
        """tile_hint of a deep-level GEMM on the rows of x [B,H,W,c]: for a batch on the bf16-rows route, the configuration ONE image's
        rows pick (ff_gemm_rows_bf16's rule counts workgroups, so it depends on the row count); 0 = the kernel's own choice otherwise.
        (The split-bf16 route's rule, ff_conv2d_bf16s_tile, does not depend on the row count for these widths: N % 128 == 0.)"""
        if not rows or x.shape[0] == 1:
            return 0
        return int(ops._L().ff_gemm_rows_bf16_tile(x.shape[1] * x.shape[2], N))

    def forward(self, lr: T, taps: Optional[dict] = None, feats: Optional[dict] = None, out: Optional[T] = None) -> T:
        """lr [B,3,h,w] -> [B,3,4h,4w] (written into `out` when given).  feats (optional dict): receives feats["nafnet"], the input of
        the ending convolution [B,Hp,Wp,64] (NHWC), the tensor the reference's forward hook captures (expert_loader.py:866).
        B > 1: one launch per op for the whole batch in the fused modes (chunks of max_batch_pixels padded HR pixels), the per-image
        loop in f32 mode (its conv3 folds sca into a dynamic weight); either way bit-equal to B single forwards.  taps are recorded
        for B == 1 only."""
        B, _, h, w = lr.shape
        m = 2 ** len(self.enc_n)
        Hp, Wp = _ceil_to(4 * h, m), _ceil_to(4 * w, m)

        def chunk(x, tp, ft, o, fo, cap):
            # the kernels take 16-byte aligned images: a slice of the batch at an odd offset is copied.  cap < B exactly when x is
            # such a slice (_forward_batch passes the whole batch with cap == B); the whole batch is never copied, as before
            return self._forward_chunk(x.clone() if cap < B and x.data_ptr() % 16 else x, tp, ft, o, cap, fo)
        return _forward_batch("NafnetHIP", "nafnet", lr, taps, feats, out,
                              lambda: min(int(self.max_batch_pixels) // (Hp * Wp), (2 ** 31 - 1) // (Hp * Wp * 64)),
                              (B, Hp, Wp, self.ending[0].shape[1] // 9), chunk)

    def _forward_chunk(self, lr: T, taps: Optional[dict], feats: Optional[dict], out: Optional[T], cap: int, feat_out: Optional[T]) -> T:
        """One launch per op for all of lr [B,3,h,w] (per_image matters for B > 1 only: ops.conv2d); cap: the largest chunk's images;
        feat_out: where the hooked feature -- the last block's output -- goes (a slice of the batch's buffer)."""
        B, _, h, w = lr.shape
        H, W = 4 * h, 4 * w
        m = 2 ** len(self.enc_n)
        Hp, Wp = _ceil_to(H, m), _ceil_to(W, m)
        inp = self._padded_input(B, Hp, Wp, lr.device, cap)
        ops.resize(lr, (H, W), mode="bicubic", scale_factor=4.0, layout="nchw", out=inp)
        x = ops.conv2d(inp, *self.intro, ksize=(3, 3), pad=(1, 1), per_image=True)
        skips = []
        for lvl, blks in enumerate(self.encs):
            for b, k in enumerate(blks):
                x = self.block(x, k)
                if taps is not None and lvl == 0:
                    taps[f"naf.enc0.b{b}"] = x
            skips.append(x)
            x = ops.conv2d(x, *self.downs[lvl], ksize=(2, 2), stride=(2, 2), pad=(0, 0), per_image=True)
        for k in self.mids:
            x = self.block(x, k)
        if taps is not None:
            taps["naf.mid"] = x
        for lvl, blks in enumerate(self.decs):
            x = ops.conv2d(x, self.ups[lvl], None, shuffle=2, res=skips[-1 - lvl], per_image=True)
            for i, k in enumerate(blks):
                x = self.block(x, k, out=feat_out if lvl == len(self.decs) - 1 and i == len(blks) - 1 else None)
        if feats is not None:
            feats["nafnet"] = x                                # expert_loader.py:866: the INPUT of the ending conv, [B,Hp,Wp,64]
        x = ops.conv2d(x, *self.ending, ksize=(3, 3), pad=(1, 1), res=inp, per_image=True)
        return ops.nhwc_to_nchw(x, H, W, clamp01=True, out=out)
