/* C ABI of libff_hip.so -- the MI355X (gfx950) kernel library behind the FreqFusion x4 inference path.
 *
 * Boundary contract.  The reference has no FFI: its "operators" are the ATen ops
 * PyTorch dispatches from models/team29_FreqFusion/io.py:221 -> src/models/enhanced_fusion.py:694-754.
 * Each entry point below replaces one cluster of those ATen ops (cited per function); the Python host
 * (image-super-resolution-2_amd/*.py) binds them with ctypes, exactly as a reference maintainer would
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain pointers + sizes, no torch types.  All tensors are fp32 DEVICE pointers owned by the caller;
 *     the library allocates nothing and keeps no state (workspaces are passed in).
 *   - activations are NHWC / token-major: element (b, y, x, c) at ((b*H + y)*W + x)*ld + c.  `ld*`
 *     arguments are row (pixel) strides in floats, so channel slices of wider tensors are addressed in place.
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); every call is asynchronous
 *     on it and graph-capturable (no allocation, no synchronisation inside).
 *   - entry points may be called with any device current (the stream's) and from several threads at once.
 *   - return 0 on success; otherwise nothing was launched and ff_last_error() describes why.
 */
#ifndef FF_KERNELS_H
#define FF_KERNELS_H
#ifdef __cplusplus
extern "C" {
#endif

#define FF_ACT_NONE 0
#define FF_ACT_GELU 1    /* exact erf GELU (nn.GELU default) */
#define FF_ACT_RELU 2
#define FF_ACT_LRELU 3   /* negative slope 0.01 (nn.LeakyReLU default) */
#define FF_ACT_SIGMOID 4

const char* ff_last_error(void);
int ff_abi_version(void);
int ff_device_cu_count(void);

/* Implicit-GEMM convolution / GEMM on fp32 MFMA:
 *   out[m][n] = res[m][n] + alpha * mul[n] * act( sum_k A[m][k] * w[n][k] + bias[n] )
 * A gathered from in[B][H][W][ldi] (channels [0,Cin), zero padding); w is [Cout][KH*KW*Cin] with
 * k = (ky*KW + kx)*Cin + ci.  bias / mul / res may be NULL.  shuffle = 2 folds nn.PixelShuffle(2) into the
 * store (out/res are then [B][2Ho][2Wo][ld] with Cout/4 channels).  A GEMM on rows [M][K] is
 * B=1,H=1,W=M,KH=KW=1.  tile_hint 0 = auto.
 * Replaces nn.Linear / nn.Conv2d (+bias +GELU/ReLU/LeakyReLU/Sigmoid +residual +PixelShuffle):
 * hat_arch.py:67-69,83-94,172,194,608,699-700,859; dat_arch.py:163-168,501,559,792,964;
 * nafnet_arch.py:77,82,95,96,160,162,174,184-185; hierarchical_fusion.py:96-127; enhanced_fusion.py:266-290;
 * edge_enhancement.py:100-180; fusion_network.py:179-197,553-576; large_kernel_attention.py:75,131-135,191-205. */
int ff_conv2d(const float* in, const float* w, const float* bias, const float* mul, const float* res, float* out,
              int B, int H, int W, int Cin, int ldi, int Ho, int Wo, int Cout, int ldo, int ldr, int KH, int KW,
              int sy, int sx, int py, int px, int act, float alpha, int shuffle, int tile_hint, void* stream);

/* Same contraction on the bf16 matrix cores with split operands ("bf16x3", csrc/conv_gemm_bf16.hip):
 * a*w ~= a_hi*w_hi + a_lo*w_hi + a_hi*w_lo, every term one v_mfma_f32_32x32x16_bf16 into the same fp32
 * accumulator.  nterms 3 = fp32-grade (~1e-5 rel), 2 = exact activations x bf16 weights, 1 = plain bf16.
 * w_hi / w_lo are bf16 planes [Cout][Kp] made by ff_split_bf16 (lo may be NULL for nterms < 3), zero filled, in one of
 * two K layouts: flat (Cp = 0, Kp = ceil32(KH*KW*Cin)) or per-tap padded (Cp = ceil32(Cin), Kp = KH*KW*Cp; needs
 * Cin % 4 == 0).  Everything else as ff_conv2d, plus two fusions of NAFBlock (nafnet_arch.py:88-106):
 *   kmul (optional, 1x1 only): [Cin] scale of the input channels, out = W (kmul * a) + ... -- conv3(x * sca) without rescaling W;
 *   shuffle = 1: SimpleGate in the epilogue, out[m][j] = y[m][2j] * y[m][2j+1] with y = A w^T + bias (Cout / 2 channels out; the
 *   caller interleaves the weight rows of the two chunk(2) halves; no residual / scale / activation). */
int ff_conv2d_bf16s(const float* in, const void* w_hi, const void* w_lo, int Kp, int Cp, const float* bias, const float* mul,
                    const float* res, float* out, int B, int H, int W, int Cin, int ldi, int Ho, int Wo, int Cout,
                    int ldo, int ldr, int KH, int KW, int sy, int sx, int py, int px, int act, float alpha, int shuffle,
                    int nterms, int tile_hint, const float* kmul, void* stream);
/* The tile configuration ff_conv2d_bf16s picks when tile_hint <= 0, from M = B * Ho * Wo, Cout, K = KH * KW * Cin and vec4 (Cin % 4 == 0,
 * 16-byte aligned input rows).  A caller that batches independent images passes the value for ONE image's M as tile_hint, so that the
 * batched launch takes the kernel form the single-image launch takes.  Added under ABI version 7 (an additive entry point). */
int ff_conv2d_bf16s_tile(long long M, int Cout, int K, int vec4);
/* conv3 of B independent images in one launch (1x1; NAFBlock conv3(g * sca) at the deep levels, split-bf16 modes).  in is fp32
 * [M][ldi] rows with M == B * rows_per_image < 2^31: rows b * rows_per_image .. (b + 1) * rows_per_image - 1 are image b's.  kmul is
 * [B][Cin], image b's scale vector at kmul + b * Cin, and row m is scaled by kmul[m / rows_per_image] before the split.  Epilogue:
 * out = (A w^T + bias) * mul + res (Cout % 4 == 0, 16-byte aligned out / res rows).  Every row is bit-equal to ff_conv2d_bf16s(1x1,
 * kmul = kmul + b * Cin) on its image alone: the kernel is that one with the image of each A row (B = B, H = 1, W = rows_per_image)
 * indexing kmul, and tile_hint <= 0 takes ff_conv2d_bf16s_tile(rows_per_image, ...), ONE image's configuration (3, 4, 5 or 7).
 * Added under ABI version 7 (an additive entry point: no existing prototype changed). */
int ff_conv2d_bf16s_kmul_images(const float* in, int ldi, const void* w_hi, const void* w_lo, int Kp, int Cp, const float* kmul, int B,
                                int rows_per_image, const float* bias, const float* mul, const float* res, int ldr, float* out, int ldo,
                                long long M, int Cin, int Cout, int nterms, int tile_hint, void* stream);
int ff_split_bf16(const float* w, int N, int K, int Kp, int Cin, int Cp, void* hi, void* lo, void* stream);

/* A 1x1 GEMM over B images with one weight matrix PER IMAGE: in [M][ldi], M == B * rows_per_image (rows_per_image % 256 == 0: no m-tile
 * straddles two images), planes w_hi / w_lo [B][Cout][Kp] (ff_split_bf16 on the [B * Cout][Cin] matrix).  Same K order and epilogue
 * ((acc + bias) * mul + res, 16-byte rows) as ff_conv2d_bf16s: every row is bit-equal to the single call on its image with its planes;
 * tile_hint <= 0 takes ff_conv2d_bf16s_tile of ONE image's rows.  DAT's att = v . wbd^T.  Added under ABI version 7 (additive). */
int ff_conv2d_bf16s_wimages(const float* in, int ldi, const void* w_hi, const void* w_lo, int Kp, int Cp, int B, int rows_per_image,
                            const float* bias, const float* mul, const float* res, int ldr, float* out, int ldo, long long M, int Cin,
                            int Cout, int nterms, int tile_hint, void* stream);

/* GEMM on bf16 ROWS, plain bf16 (csrc/gemm_rows_bf16.hip): out[M][N] = epilogue(A[M][K] . W[N][K]^T), bit-equal to
 * ff_conv2d_bf16s(1x1, nterms = 1) on the fp32 upcast of A -- the same MFMA, k order and epilogue arithmetic -- with both operands
 * fetched by LDS-DMA.  a: bf16 [M][lda]; w_hi: the hi plane of ff_split_bf16 [N][Kp].  Needs K % 64 == 0, Kp == K, lda % 8 == 0
 * and 16-byte aligned a / w_hi.  bias / mul / res may be NULL.
 * a_fp32 = 1: a is fp32 [M][lda] (lda % 4 == 0), staged through registers and rounded on the way as ff_conv2d_bf16s does; only then may
 * kmul [K] be given, the per-input-channel fp32 scale of A (conv3(x * sca)); gate = 0 only.
 *   gate = 0: out fp32 [M][ldo] = (A w^T + bias) * mul + res   (N % 4 == 0, ldo / ldr % 4 == 0, 16-byte aligned out / res);
 *   gate = 1: SimpleGate on interleaved columns, out bf16 [M][ldo] with N / 2 channels, out[m][j] = bf16(y[m][2j] * y[m][2j+1])
 *             (N % 8 == 0, ldo % 4 == 0, no mul / res): what ff_conv2d_bf16s(shuffle = 1) stores, rounded once.
 * tile_hint 0 = auto; 1 / 2 = the 128x128 / 128x64 tile.
 * NAFBlock conv1 / conv3 / conv4 / conv5 at 256 / 512 / 1024 channels (nafnet_arch.py:77,95,96).  Added under ABI version 7 (an additive
 * entry point: no existing prototype changed). */
int ff_gemm_rows_bf16(const void* a, int a_fp32, int lda, const void* w_hi, int Kp, const float* kmul, const float* bias,
                      const float* mul, const float* res, int ldr, void* out, int ldo, long long M, int N, int K, int gate,
                      int tile_hint, void* stream);
/* The tile configuration ff_gemm_rows_bf16 picks when tile_hint <= 0, from M and N.  A caller that batches independent images passes the
 * value for ONE image's M as tile_hint.  Added under ABI version 7 (an additive entry point). */
int ff_gemm_rows_bf16_tile(long long M, int N);
/* ff_gemm_rows_bf16(a_fp32 = 1, gate = 0) for B independent images in one launch: a fp32 [M][lda], M == B * rows_per_image < 2^31, rows
 * b * rows_per_image .. of a / res / out are image b's; kmul is [B][K], image b's vector at kmul + b * K, and row m is scaled by
 * kmul[m / rows_per_image] before the bf16 rounding (looked up per staged row, so an m-tile may hold rows of several images and the
 * tiling is the single-image kernel's).  Every row is bit-equal to ff_gemm_rows_bf16(kmul = kmul + b * K) on its image alone.
 * tile_hint <= 0 takes ff_gemm_rows_bf16_tile(rows_per_image, N).  Added under ABI version 7 (an additive entry point). */
int ff_gemm_rows_bf16_kmul_images(const float* a, int lda, const void* w_hi, int Kp, const float* kmul, int B, int rows_per_image,
                                  const float* bias, const float* mul, const float* res, int ldr, float* out, int ldo, long long M,
                                  int N, int K, int tile_hint, void* stream);

/* 3x3 / stride 1 / pad 1 convolution for small channel counts (csrc/conv3x3_small.hip): Cin <= 64, Cout <= 16, exact fp32 on
 * the VALU, out = res + alpha * act(conv(in) + bias).  w_small: fp32 [9][ceil4(Cin)][CT], CT = 1 / 4 / 16 >= Cout, zero padded
 * (prep.pack_conv3x3_small).  Replaces the tail convolutions of the fusion stack at 1024 x 1024: to_rgb (hierarchical_fusion.py:
 * 124-128), refine_net.6 (enhanced_fusion.py:288), the edge fusion / gate convolutions (edge_enhancement.py:112,170-180). */
int ff_conv3x3_small(const float* in, int ldi, const float* w_small, int ct, const float* bias, const float* res, int ldr,
                     float* out, int ldo, int B, int H, int W, int Cin, int Cout, int act, float alpha, void* stream);


/* Fused window attention softmax((q*scale) k^T + bias (+mask)) v on fp32 MFMA; one workgroup per
 * (window, head).  qkv is the token tensor [B][H][W][ldq]; q/k/v of head h live at *_off + h*d.
 * Queries: wh x ww windows (wh*ww == 256) on the (Hp, Wp) zero-padded grid, cyclically shifted by
 * (shift_h, shift_w); keys: kh x kw window centred on the query window (zero outside the image).
 * biasT is [heads][kh*kw][256] (key-major).  use_mask adds the -100 shifted-window region mask.
 * Output written un-shifted and cropped at out[token][o_off + h*d ..].
 * Replaces hat_arch.py:97-126,165-196,280-303 (+mask :921-940), :400-433 (OCAB unfold path),
 * dat_arch.py:62-96,269-342,505-548. */
int ff_window_attn(const float* qkv, int ldq, int q_off, int k_off, int v_off, float* out, int ldo, int o_off,
                   const float* biasT, int B, int H, int W, int Hp, int Wp, int wh, int ww, int kh, int kw,
                   int shift_h, int shift_w, int use_mask, int heads, int d, float scale, void* stream);

/* Same attention on the bf16 matrix cores with split operands (csrc/attention_bf16.hip): nterms 3 = fp32-grade
 * (hi*hi + lo*hi + hi*lo for both QK^T and PV), 1 = plain bf16 operands.  Same arguments otherwise, except that the
 * bias table is quad-interleaved: biasT[head][key / 4][query][key % 4] (= the table of ff_window_attn reshaped
 * [heads][nk/4][4][256] and permuted (0,1,3,2); prep.quad_bias), so four consecutive keys of a query are one 16-byte load.
 * kh*kw % 4 == 0.
 * rel_table (optional, may be NULL): the compact relative-position table [heads][(2wh-1)*(2ww-1)] with
 *   bias[q][k] = rel_table[head][(qy - ky + wh - 1)*(2ww - 1) + (qx - kx + ww - 1)]     (hat_arch.py:882-899, dat_arch.py:300-318)
 * gathered from LDS instead of streaming the expanded table (then biasT may be NULL); needs keys == query window and a
 * power-of-two window width. */
int ff_window_attn_bf16s(const float* qkv, int ldq, int q_off, int k_off, int v_off, float* out, int ldo, int o_off,
                         const float* biasT, int B, int H, int W, int Hp, int Wp, int wh, int ww, int kh, int kw,
                         int shift_h, int shift_w, int use_mask, int heads, int d, float scale, int nterms, const float* rel_table,
                         void* stream);

/* Attention output projection + residuals + norm2 + MLP in one launch (csrc/token_mlp.hip, token_projmlp_kernel):
 *   x1 = x + proj(att) + c2 * c2_scale;  out = x1 + fc2(GELU(fc1(LayerNorm(x1))))        (hat_arch.py:303-307, OCAB :434-437)
 * x1 never reaches memory.  proj_tiles / proj_bias_padded: ff_token_linear's weight format for the 180 -> 180 projection;
 * mlp_tiles: ff_token_mlp's format with fc1's K columns in the accumulator-operand order (prep.pack_token_projmlp);
 * c2 / c2_scale may be NULL (no convolution branch).  K = N <= 192.
 * nterms (here and in every token / halo / NAFNet kernel below): 3 = split-bf16 products hi*lo + lo*hi + hi*hi (fp32-grade results),
 * 1 = plain bf16 operands (hi*hi only: a third of the MFMAs; the weight images are the same, their lo planes unused).
 * io_bf16 (nterms == 1 only; the pointers are then bf16 rows with the pitch in elements): bit 0 = att, bit 1 = c2.  An intermediate
 * whose only consumer rounds it to bf16 as an MFMA operand can be stored as bf16 with bit-identical results (att, the normalised rows
 * of ff_win_attn_fused, conv1's output inside CAB); c2 enters x1 times conv_scale = 0.01, where the rounding is 2e-5 of x1. */
int ff_token_projmlp(const float* att, int lda, const float* x, int ldx, const float* c2, int ldc, const float* c2_scale,
                     float* out, int ldo, long long M, int K, int hidden_tiles, const void* proj_tiles,
                     const float* proj_bias_padded, const float* gamma, const float* beta, float eps,
                     const void* mlp_tiles, const float* b1_padded, const float* b2, int nterms, int io_bf16, void* stream);
/* ff_token_projmlp over a batch of B images with ONE GATE PER IMAGE (HAT's channel attention is per image): c2_scale is [B][scale_ld]
 * (scale_ld >= K, scale_ld % 4 == 0) and image b -- tokens b * rows_per_image .. (b + 1) * rows_per_image - 1 -- computes
 *   x1 = x + proj(att) + c2 * c2_scale[b].
 * A workgroup owns 256 consecutive tokens, so rows_per_image % 256 == 0 and M == B * rows_per_image are required (anything else is
 * refused before the launch; HAT pads to multiples of 16 pixels, i.e. of 256 tokens).  The grid is (rows_per_image / 256, B): the image
 * index is blockIdx.y, uniform per workgroup, no vector register and no division.  Every token's arithmetic is that of ff_token_projmlp,
 * so the result is bit-equal to B calls on the row slices, and B == 1 makes the launch ff_token_projmlp makes.  c2 and c2_scale are
 * required.  Added under ABI version 7 (an additive entry point: no existing prototype changed). */
int ff_token_projmlp_images(const float* att, int lda, const float* x, int ldx, const float* c2, int ldc, const float* c2_scale,
                            int scale_ld, int B, long long rows_per_image, float* out, int ldo, long long M, int K,
                            int hidden_tiles, const void* proj_tiles, const float* proj_bias_padded, const float* gamma,
                            const float* beta, float eps, const void* mlp_tiles, const float* b1_padded, const float* b2,
                            int nterms, int io_bf16, void* stream);

/* Window-resident attention block (csrc/win_attn_fused.hip): LayerNorm -> q/k/v projection -> softmax(q k^T + bias (+mask)) v
 * for ALL `nheads` heads of one 256-token window per workgroup; the qkv tensor never exists in memory.
 * Replaces, in one launch, HAB's norm1 + roll + window_partition + WindowAttention.forward up to the output projection
 * (hat_arch.py:272-303 with :165-192) and DAT's qkv + one SpatialAttention branch (dat_arch.py:501-548 with :290-342).
 *   x [tokens][ldx] (K <= 192 channels), gamma/beta: LayerNorm (NULL: none), eps.
 *   w_tiles: bf16 [3*heads_total][2 planes hi,lo][32][192]: tile 3g+0/1/2 = the q / k / v rows of head g (head dim padded
 *     to 32 rows, K to 192 columns, zero filled; the softmax scale is folded into the q rows and bias);
 *     bias_padded [3*heads_total*32] (prep.pack_win_attn).
 *   rel_padded [heads_total][2wh-1][stride]: compact relative-position bias,
 *     bias[q][k] = rel[head][(qy - ky + wh - 1)*stride + (qx - kx + ww - 1)], stride 40 / 48 / 64 for ww 8 / 16 / 32.
 *   Window wh x ww = 256 tokens (ww 8, 16 or 32), keys = the query window; cyclic shift + region mask as ff_window_attn.
 *   Heads head0 .. head0+nheads-1 are processed; head g writes out[token][o_off + g*d .. +d).
 *   zero_pad_tokens != 0: q/k/v of tokens outside H x W are exactly zero (DAT pads AFTER the projection, dat_arch.py:515-520);
 *   0: such tokens do not occur (HAT pads the image beforehand).
 *   xn_out (optional): the LayerNorm'ed rows [tokens][ldxn] (HAT's conv branch input, hat_arch.py:274).
 *   v_out (optional): v of the processed heads, v_out[token][v_off + g*d ..) (DAT's depth-wise conv branch, dat_arch.py:524).
 * nterms 3 = split-bf16 (fp32-grade), 1 = plain bf16.  out_bf16 / xn_bf16 (nterms == 1 only): out / xn_out are bf16 rows, pitches in
 * elements (xn rows padded to a multiple of 8). */
int ff_win_attn_fused(const float* x, int ldx, float* out, int ldo, int o_off, const float* gamma, const float* beta,
                      float eps, const void* w_tiles, const float* bias_padded, const float* rel_padded, int rel_rows,
                      int rel_stride, int B, int H, int W, int Hp, int Wp, int wh, int ww, int shift_h, int shift_w,
                      int use_mask, int head0, int nheads, int d, int K, int zero_pad_tokens, float* xn_out, int ldxn,
                      float* v_out, int ldv, int v_off, int nterms, int out_bf16, int xn_bf16, void* stream);

/* HAB link, plain bf16 (csrc/hab_link.hip): block i's ff_token_projmlp_images and block i+1's ff_win_attn_fused in ONE launch.
 *   x_out = x1 + fc2(GELU(fc1(LayerNorm2(x1)))),  x1 = x + proj(att) + c2 * c2_scale[image]        (the first 25 arguments: those of
 *                                                                                                   ff_token_projmlp_images)
 *   xn_out = LayerNorm1(x_out),  att_out = (S)W-MSA of all six heads on xn_out                      (the rest: those of ff_win_attn_fused
 *                                                                                                   with head0 = 0, Hp = H, Wp = W, no v_out)
 * A workgroup is one (shifted) 16 x 16 window of block i+1; the final x of its 256 tokens passes from the MLP's accumulators to the
 * attention's LayerNorm through LDS, so the attention never reads x_out back.  x_out is still written (block i+1's residual).  Every
 * statement of the arithmetic is the parents', in their order: all three outputs are BIT EQUAL to the two launches.
 * Refused before any launch (FF_ERR_ARG): nterms != 1; a window other than 16 x 16; d != 30 or nheads != 6; K != 180; H or W not a
 * multiple of 16; io_bf16 != 3, out_bf16 != 1 or xn_bf16 != 1 (att, c2, xn_out and att_out are bf16 rows, pitches in elements; att and
 * xn rows padded to 192); c2 or c2_scale NULL; rows_per_image != H * W or M != B * rows_per_image; more than 12 hidden tiles; rows or
 * weights that miss the alignment of the parents; B * H * W * ld >= 2^31 for any pitch.
 * Added under ABI version 7 (an additive entry point: no existing prototype changed). */
int ff_hab_link(const float* att, int lda, const float* x, int ldx, const float* c2, int ldc, const float* c2_scale,
                int scale_ld, int B, long long rows_per_image, float* x_out, int ldxo, long long M, int K, int hidden_tiles,
                const void* proj_tiles, const float* proj_bias_padded, const float* gamma2, const float* beta2, float eps2,
                const void* mlp_tiles, const float* b1_padded, const float* b2, int nterms, int io_bf16,
                float* att_out, int ldo, int o_off, const float* gamma1, const float* beta1, float eps1,
                const void* qkv_tiles, const float* qkv_bias_padded, const float* rel_padded, int rel_rows, int rel_stride,
                int H, int W, int wh, int ww, int shift_h, int shift_w, int use_mask, int nheads, int d,
                float* xn_out, int ldxn, int out_bf16, int xn_bf16, void* stream);

/* Fused transformer feed-forward on tokens (csrc/token_mlp.hip): out = x + fc2(GELU(fc1(LayerNorm(x)))), bf16x3 MFMA.
 * Replaces hat_arch.py:307 (norm2 + Mlp.forward :88-94 + residual) in one launch; the hidden activation stays on chip.
 * K, N <= 192.  w_tiles: bf16 [hidden_tiles][4][6144] = per 32-wide hidden tile the planes W1_hi, W1_lo ([32][192], zero
 * padded) and W2_hi, W2_lo ([192][32], hidden column stored at position p = index with bits 2 and 3 swapped)
 * (prep.pack_token_mlp); b1 zero padded to hidden_tiles*32; gamma/beta/w_tiles 16-byte aligned. */
int ff_token_mlp(const float* x, int ldx, float* out, int ldo, long long M, int K, int hidden_tiles, int N,
                 const float* gamma, const float* beta, float eps, const void* w_tiles, const float* b1_padded,
                 const float* b2, int nterms, void* stream);

/* 3x3 / stride 1 / pad 1 convolution with the input tile resident in LDS (csrc/conv3x3_halo.hip), bf16x3 MFMA:
 *   out = act(conv3x3(in) + bias) * mul[co] * alpha + res        (shuffle = 2: PixelShuffle(2) fused into the store)
 * Same arithmetic as ff_conv2d_bf16s(nterms = 3) but the (TH+2) x 18 pixel halo tile is split to bf16 hi/lo and staged
 * once per 64-channel chunk instead of once per filter tap.  Replaces nn.Conv2d(k=3, s=1, p=1) of hat_arch.py:121-130
 * (CAB), :768, :921-953; dat_arch.py:396,772; nafnet_arch.py:187,193 and the fusion stack's 3x3 convolutions.
 * bn in {32, 64, 128, 192} = output channels per workgroup.  w_img: prep.pack_conv3x3_halo image
 * [ceil(Cout/bn)][ceil(Cin/64)][9 taps][bn rows x (64 hi | 64 lo | 8 pad) bf16, padded to 1 KiB] for nterms = 3, and the compact
 * hi-only rows (64 hi | 8 pad) for nterms = 1 (then the 16x16-pixel tile is 50 KB of LDS and the 64-channel forms run two
 * workgroups per CU), of ff_conv3x3_halo_weight_bytes(Cout, Cin, bn, nterms) bytes (-1: bad arguments).  Needs Cin % 4 == 0, 16-byte aligned rows. */
long long ff_conv3x3_halo_weight_bytes(int Cout, int Cin, int bn, int nterms);
/* pool_partials (optional, Cout <= bn, no shuffle): [ff_conv3x3_halo_pool_rows(B,H,W,Cout,bn,nterms)][bn] per-workgroup channel sums of the
 * stored output, finished by ff_pool_finish (the global average pool of hat_arch.py:50 without re-reading the tensor).
 * io_bf16 (nterms == 1, no shuffle, no residual): bit 0 = `in` rows are bf16, bit 1 = `out` rows are bf16 (pitches in elements; the
 * pool partials are taken from the fp32 values before rounding). */
long long ff_conv3x3_halo_pool_rows(int B, int H, int W, int Cout, int bn, int nterms);
int ff_pool_finish(const float* part, int rows, int ld, int C, float inv_count, float* out, void* stream);
int ff_conv3x3_halo(const float* in, int ldi, const void* w_img, int bn, const float* bias, const float* mul,
                    const float* res, int ldr, float* out, int ldo, int B, int H, int W, int Cin, int Cout,
                    int act, float alpha, int shuffle, float* pool_partials, int nterms, int io_bf16, void* stream);
/* ff_conv3x3_halo over B INDEPENDENT IMAGES, each reproducing the bits of its own B == 1 launch -- output and pool partials.
 * ff_conv3x3_halo(B > 1) differs from that in two ways: it picks its kernel form (8 or 16 pixel rows per workgroup) from the tile count
 * of the whole launch, and it indexes the partial rows by workgroup after an XCD remap over ALL tiles, so an image's partial rows
 * interleave with the others' in an order that depends on B.  Here the form is the one ff_conv3x3_halo(B = 1, H, W, ...) takes, workgroup
 * w belongs to image w / wpi (wpi = workgroups of one image), the remap runs over the wpi workgroups of that image, and the partial goes
 * to row w: rows b * wpi .. (b + 1) * wpi - 1 of pool_partials [ff_conv3x3_halo_images_pool_rows(B, ...)][bn] are image b's single-image
 * rows in their single-image order (finish them with ff_pool_vec_mlp_images, or ff_pool_finish per image).  Same arguments and
 * restrictions as ff_conv3x3_halo otherwise.  Added under ABI version 7 (additive entry points). */
long long ff_conv3x3_halo_images_pool_rows(int B, int H, int W, int Cout, int bn, int nterms);
int ff_conv3x3_halo_images(const float* in, int ldi, const void* w_img, int bn, const float* bias, const float* mul,
                           const float* res, int ldr, float* out, int ldo, int B, int H, int W, int Cin, int Cout,
                           int act, float alpha, int shuffle, float* pool_partials, int nterms, int io_bf16, void* stream);

/* HAT's CAB in one launch (csrc/cab_fused.hip), plain bf16 only: c2 = conv3x3(gelu(conv3x3(xn) + bias1)) + bias2 on bf16 rows, c1 kept
 * in LDS.  xn [B][H][W][ldi] and c2 [B][H][W][ldo] are bf16 rows (io_bf16 must be 3, pitches in elements, ldi % 8 == 0, ldo % 4 == 0),
 * w1_img / w2_img are the nterms = 1 images of prep.pack_conv3x3_halo for (Cmid, Cin, bn 64) and (Cout, Cmid, bn 192) and w1_bytes /
 * w2_bytes their sizes, which must be ff_conv3x3_halo_weight_bytes of those shapes.  pool_partials
 * [ff_conv3x3_halo_images_pool_rows(B, H, W, Cout, 192, 1)][192]: image b's rows at b * (rows / B).  c2 and the partial rows are bit for
 * bit those of ff_conv3x3_halo_images(xn -> c1, gelu, bf16 rows) followed by ff_conv3x3_halo_images(c1 -> c2, pool partials).
 * Refused: nterms != 1, rows that are not bf16, channels other than 180 -> 60 -> 180, H or W not a multiple of 16, H * W < 1024, pitches or
 * addresses the 16-byte paths cannot take, weight images of another size, B * H * W * pitch >= 2^31, c2 aliasing xn.
 * Added under ABI version 7 (additive entry point). */
int ff_cab_fused(const void* xn, int ldi, const void* w1_img, long long w1_bytes, const float* bias1,
                 const void* w2_img, long long w2_bytes, const float* bias2, void* c2, int ldo, float* pool_partials,
                 int B, int H, int W, int Cin, int Cmid, int Cout, int nterms, int io_bf16, void* stream);

/* Token-stationary linear layer for K <= 192 (csrc/token_linear.hip), bf16x3 MFMA:
 *   out = res + res2*res2_scale[n] + act( LayerNorm?(x) . W^T + bias )        (gamma == NULL: no LayerNorm)
 * x is read once and kept in registers, W streams through LDS by DMA.  Replaces nn.LayerNorm + nn.Linear (+GELU,
 * +residuals): hat_arch.py:272+172 (OCAB :397+400), :194+306; dat_arch.py:734+501, :559, :735+163.
 * kpad = K rounded up to 64 / 128 / 192.  w_tiles: bf16 [n_tiles][2][32][kpad] (hi, lo planes; rows >= N and cols >= K
 * zero) from prep.pack_token_linear;
 * bias zero padded to n_tiles*32 (or NULL).  xn_out (optional, needs gamma): the LayerNorm'ed rows are also written there
 * (row pitch ldxn), which saves the separate ff_layernorm pass when another consumer needs them (HAT's CAB branch).  * stats_out (optional) [M][2]: per token (mean, 1/sqrt(var + stat_eps)) of the activated OUTPUT channels [stat_lo, stat_hi) -- the
 * LayerNorm statistics a consumer applies on load (ff_dwconv3x3_ln; DAT SpatialGate, dat_arch.py:117-122). */
int ff_token_linear(const float* x, int ldx, float* out, int ldo, long long M, int K, int kpad, int N, int n_tiles,
                    const float* gamma, const float* beta, float eps, const void* w_tiles, const float* bias_padded,
                    int act, const float* res, int ldr, const float* res2, int ldr2, const float* res2_scale,
                    float* xn_out, int ldxn, float* stats_out, int stat_lo,
                    int stat_hi, float stat_eps, int nterms, void* stream);

/* ff_token_linear with a column-scaled bf16 output (csrc/token_linear.hip, plain bf16 products only):
 *   out16[token][n] = bf16( (LayerNorm?(x) . W^T + bias)[n] * col_scale[n] )
 * -- the fp32 value ff_token_linear(nterms = 1) would store, times col_scale[n] in fp32, rounded once.  out16: bf16 rows, ldo in
 * ELEMENTS (a multiple of 4, base 8-byte aligned); col_scale [n_tiles*32], 16-byte aligned.  The parameter list is ff_token_linear's;
 * nterms != 1, act != none, res, res2, res2_scale, xn_out and stats_out are refused.  With prep.pack_ocab_qkv's weights it writes HAT
 * OCAB's q (scaled) / k / v as the head-padded rows ff_ocab_attn_rows16 reads. */
int ff_token_linear_rows16(const float* x, int ldx, void* out16, int ldo, long long M, int K, int kpad, int N, int n_tiles,
                           const float* gamma, const float* beta, float eps, const void* w_tiles, const float* bias_padded,
                           const float* col_scale, int act, const float* res, int ldr, const float* res2, int ldr2,
                           const float* res2_scale, float* xn_out, int ldxn, float* stats_out, int stat_lo,
                           int stat_hi, float stat_eps, int nterms, void* stream);

/* ff_token_linear with DAT's adaptive-interaction prologue (csrc/token_linear.hip, GATED): the GEMM input is
 *   x * cm[channel] + x2 * sm[token],   sm = sigmoid(gw2 . gelu(GW1 x + gb1) + gb2)
 * i.e. the channel gate on one branch, the spatial gate (conv1x1 180->11 (+BN folded) -> GELU -> conv1x1 11->1 -> sigmoid,
 * dat_arch.py:585-590) computed from that same branch and applied to the other, then the output projection + bias + residual
 * (dat_arch.py:541-559 spatial blocks with x = attention, x2 = conv; :649-666 channel blocks with x = conv, x2 = attention).
 * w_tiles: prep.pack_token_linear_gated = the projection's tiles followed by ONE more 32-row tile holding GW1 (rows 11..31 zero);
 * gb1 / gw2: [32] zero padded.  Replaces ff_pixel_mlp + ff_mix2 + ff_token_linear and the 47 MB tensor between them. */
int ff_token_linear_gated(const float* x, int ldx, const float* x2, int ldx2, const float* cm, const float* gw1t, const float* gb1,
                          const float* gw2, float gb2, float* out, int ldo, long long M, int K, int N, int n_tiles,
                          const void* w_tiles, const float* bias_padded, const float* res, int ldr, int nterms, void* stream);
/* ff_token_linear_gated over B images of rows_per_image tokens (a multiple of 256: a workgroup's 256 tokens are one image's) with one
 * channel gate per image, cm [B][K]; M == B * rows_per_image.  Bit-equal to B single calls.  Added under ABI version 7 (additive). */
int ff_token_linear_gated_images(const float* x, int ldx, const float* x2, int ldx2, const float* cm, int B, long long rows_per_image,
                                 const float* gb1, const float* gw2, float gb2, float* out, int ldo, long long M, int K, int N, int n_tiles,
                                 const void* w_tiles, const float* bias_padded, const float* res, int ldr, int nterms, void* stream);

/* NAFNet block fusions (csrc/naf_fused.hip).
 * ff_dwconv3_gate_pool: out[p][c] = dw3x3(in)[p][c] * dw3x3(in)[p][C + c] (conv2 + SimpleGate, nafnet_arch.py:78-81,51-52)
 *   and pooled[c] = mean_p out[p][c] (the SCA pool, :86) in one pass.  in [H][W][ldi] with 2C channels, weights tap-major
 *   [9][2C], bias [2C]; work: ff_dwconv3_gate_pool_workspace(C) floats.
 * ff_naf_ffn: out = y + out_scale[n] * (W5 . SimpleGate(W4 . LayerNorm(y) + b4) + b5)   (nafnet_arch.py:124-131), C = 64 / 128,
 *   bf16x3 MFMA, hidden activation on chip.  w_tiles from prep.pack_naf_ffn. */
long long ff_dwconv3_gate_pool_workspace(int C);
int ff_dwconv3_gate_pool(const float* in, int ldi, float* out, int ldo, int H, int W, int C, const float* w_tapmajor,
                         const float* bias, float* pooled, float* work, long long work_floats, void* stream);
/* ff_dwconv3_gate_pool on B independent images in one launch: in [B][H][W][ldi], out [B][H][W][ldo] (image strides H * W * ld),
 * pooled [B][C].  Grid (nb, B) with nb ONE image's workgroup count (its 1024 cap included): every image keeps its own item-to-workgroup
 * assignment and summation order, so it comes out with the bits of ff_dwconv3_gate_pool on it alone, whatever B is.  work >=
 * ff_dwconv3_gate_pool_images_workspace(B, C) = B x the single-image value (-1 for B < 1) floats, laid out [B][nb][C].
 * Added under ABI version 7 (additive entry points). */
long long ff_dwconv3_gate_pool_images_workspace(int B, int C);
int ff_dwconv3_gate_pool_images(const float* in, int ldi, float* out, int ldo, int B, int H, int W, int C, const float* w_tapmajor,
                                const float* bias, float* pooled, float* work, long long work_floats, void* stream);

/* NAFBlock front half in one launch (csrc/naf_front.inc; nafnet_arch.py:88-98) for C = 64 / 128:
 *   g = SimpleGate(dw3x3(conv1(LayerNorm2d(x)))), pooled = mean over pixels of g (SCA's average pool).
 * x [H*W][ldx] (C channels), out [H*W][ldo] (C channels), w1_tiles = prep.pack_token_linear image of conv1 [2C, C] (bf16 hi/lo 32-row
 * tiles), b1 [2C], dw_tapmajor [9][2C], dw_bias [2C], work >= ff_naf_front_workspace(H, W, C) floats.  Replaces ff_token_linear
 * (LayerNorm + conv1) followed by ff_dwconv3_gate_pool: the 2C-wide tensor between them never reaches memory. */
long long ff_naf_front_workspace(int H, int W, int C);
int ff_naf_front(const float* x, int ldx, int H, int W, int C, const float* ln_gamma, const float* ln_beta, float eps,
                 const void* w1_tiles, const float* b1, const float* dw_tapmajor, const float* dw_bias, float* out, int ldo,
                 float* pooled, float* work, long long work_floats, int nterms, void* stream);
/* ff_naf_front on B independent images in one launch: x [B][H*W][ldx], out [B][H*W][ldo] (image strides H * W * ld), pooled [B][C].
 * Grid (tiles, B): the image is blockIdx.y, the tile index and its XCD remap are those of one image's launch.  work >=
 * ff_naf_front_images_workspace(B, H, W, C) = B x the single-image value (-1 for B < 1) floats: partial rows [B][tiles][C], each image's
 * in its single-image order, finished per image in that order.  Image b has the bits of ff_naf_front on it alone.
 * Added under ABI version 7 (additive entry points). */
long long ff_naf_front_images_workspace(int B, int H, int W, int C);
int ff_naf_front_images(const float* x, int ldx, int B, int H, int W, int C, const float* ln_gamma, const float* ln_beta, float eps,
                        const void* w1_tiles, const float* b1, const float* dw_tapmajor, const float* dw_bias, float* out, int ldo,
                        float* pooled, float* work, long long work_floats, int nterms, void* stream);
int ff_naf_ffn(const float* y, int ldy, float* out, int ldo, long long M, int C, const float* gamma_ln, const float* beta_ln,
               float eps, const void* w_tiles, const float* b4, const float* b5, const float* out_scale, int nterms, void* stream);

/* NAFBlock tail in one launch (csrc/naf_tail.hip; nafnet_arch.py:118-131), plain bf16 (one MFMA term) only, C = 64 / 128:
 *   y = x + beta[n] * (W3 . (g * sca) + b3),   out = y + out_scale[n] * (W5 . SimpleGate(W4 . LayerNorm(y) + b4) + b5).
 * Bit-equal to ff_conv2d_bf16s(1x1, kmul = sca, mul = beta, res = x, nterms = 1) followed by ff_naf_ffn(nterms = 1); y never
 * reaches memory.  g, x [M][ldg / ldx] (16-byte aligned rows, ld % 4 == 0), out [M][ldo] must not alias them; sca, b3, beta,
 * gamma_ln, beta_ln, b5, out_scale [C], b4 [2C]; w_frags = prep.pack_naf_tail (W3 | W4 | W5 in MFMA fragment order, 4 C^2 bf16).
 * Added under ABI version 7 (an additive entry point: no existing prototype changed). */
int ff_naf_tail(const float* g, int ldg, const float* x, int ldx, float* out, int ldo, long long M, int C, const float* sca,
                const float* b3, const float* beta, const float* gamma_ln, const float* beta_ln, float eps, const void* w_frags,
                const float* b4, const float* b5, const float* out_scale, void* stream);
/* ff_naf_tail on the rows of B independent images in one launch: M == B * rows_per_image < 2^31, rows b * rows_per_image .. of g / x /
 * out are image b's, sca is [B][C] (16-byte aligned; image b's vector at sca + b * C, read from global memory per wave instead of the
 * LDS constant block).  rows_per_image must be a multiple of 32 -- a wave's 32 rows then belong to one image; anything else is refused
 * before the launch.  Every row is bit-equal to ff_naf_tail(sca = sca + b * C) on its image alone.
 * Added under ABI version 7 (an additive entry point: no existing prototype changed). */
int ff_naf_tail_images(const float* g, int ldg, const float* x, int ldx, float* out, int ldo, long long M, int C, const float* sca,
                       int B, int rows_per_image, const float* b3, const float* beta, const float* gamma_ln, const float* beta_ln,
                       float eps, const void* w_frags, const float* b4, const float* b5, const float* out_scale, void* stream);

/* LayerNorm over the last axis of [rows][C] (nn.LayerNorm and NAFNet LayerNorm2d in NHWC):
 * hat_arch.py:272,307,397,437,964; dat_arch.py:117,734-735,931,1003; nafnet_arch.py:35-41. */
int ff_layernorm(const float* in, int ldi, float* out, int ldo, long long rows, int C, const float* gamma,
                 const float* beta, float eps, void* stream);
/* The same LayerNorm with bf16 output rows [rows][ldo]: (bf16) of the value ff_layernorm stores, for a consumer that rounds it to
 * bf16 anyway (ff_gemm_rows_bf16's A operand).  Added under ABI version 7 (an additive entry point). */
int ff_layernorm_bf16out(const float* in, int ldi, void* out, int ldo, long long rows, int C, const float* gamma,
                         const float* beta, float eps, void* stream);

/* Global average pool over the P pixels of each of B images: out[B][C] (AdaptiveAvgPool2d(1):
 * hat_arch.py:50; dat_arch.py:411,603; nafnet_arch.py:86).  work: ff_pool_mean_workspace floats. */
int ff_pool_mean(const float* in, int ld, int B, long long P, int C, float* out, float* work, long long work_floats,
                 void* stream);
long long ff_pool_mean_workspace(int B, long long P, int C);

/* out[b] = act2(W2 . act1(W1 . in[b] + b1) + b2) * post; W2 == NULL -> single layer act1(W1.in+b1)*post.
 * The 1x1-conv MLPs that follow the pools (hat_arch.py:51-54; dat_arch.py:412-416,604-608; nafnet_arch.py:87). */
int ff_vec_mlp(const float* in, int B, int Cin, const float* W1, const float* b1, int Ch, int act1, const float* W2,
               const float* b2, int Cout, int act2, float post, float* out, void* stream);

/* First stage of ff_pool_mean alone (one image of P pixels): part[ff_pool_partial_rows(P)][C] partial sums, to be finished by
 * ff_pool_vec_mlp or ff_pool_finish (inv_count = 1 / P, ld = C). */
int ff_pool_partial_rows(long long P);
int ff_pool_partials(const float* in, int ld, long long P, int C, float* part, long long part_floats, void* stream);
/* The same for B images of P pixels each (P % 256 == 0) in one launch: part [B][ff_pool_partial_rows(P)][C], image b's rows those of its
 * own ff_pool_partials call in their order; ff_pool_partials_images_rows = B * ff_pool_partial_rows(P) (-1 for a refused geometry).
 * Finish with ff_pool_vec_mlp_images.  Added under ABI version 7 (additive). */
long long ff_pool_partials_images_rows(int B, long long P);
int ff_pool_partials_images(const float* in, int ld, int B, long long P, int C, float* part, long long part_floats, void* stream);

/* ff_pool_finish + the two-layer ff_vec_mlp in one single-workgroup launch (one image, hidden width <= 64):
 *   v[c] = inv_count * sum_r part[r][c] (r < rows, pitch ld);  out = act2(W2 . act1(W1 . v + b1) + b2) * post;
 * pooled_out (may be NULL) receives v.  The channel attention behind a conv's pool partials, hat_arch.py:50-54. */
int ff_pool_vec_mlp(const float* part, int rows, int ld, float inv_count, int Cin, const float* W1, const float* b1, int Ch,
                    int act1, const float* W2, const float* b2, int Cout, int act2, float post, float* out, float* pooled_out,
                    void* stream);
/* ff_pool_vec_mlp for B images in one launch, one workgroup per image: image b finishes the `rows` partial rows at
 * part + b * rows * ld in the summation order of the single-image launch and writes out[b][Cout] (pooled_out[b][Cin], may be NULL):
 * bit-equal to B ff_pool_vec_mlp launches.  Added under ABI version 7 (an additive entry point). */
int ff_pool_vec_mlp_images(const float* part, int B, int rows, int ld, float inv_count, int Cin, const float* W1, const float* b1,
                           int Ch, int act1, const float* W2, const float* b2, int Cout, int act2, float post, float* out,
                           float* pooled_out, void* stream);

/* HAT OCAB attention stage (hat_arch.py:392-438), plain bf16 MFMA: softmax(q k^T * scale + bias) v for 16x16 query windows against
 * the 24x24 key windows of nn.Unfold(kernel 24, stride 16, padding 4) -- keys outside the image are zero vectors that still take
 * part in the softmax.  qkv rows [B*H*W][ldq] hold q / k / v at q_off / k_off / v_off + head * 30; rel_rotated [heads][39*39] is the
 * relative_position_bias_table rotated as prep.pack_rel_overlap does (the reference gathers it with negative, wrapped indices).
 * One persistent workgroup per window; built for ws = 16, ows = 24, d = 30 (anything else: ff_window_attn_bf16s). */
int ff_ocab_attn(const float* qkv, int ldq, int q_off, int k_off, int v_off, float* out, int ldo, int o_off,
                 const float* rel_rotated, int B, int H, int W, int heads, int d, int ws, int ows, float scale, int out_bf16, void* stream);

/* ff_ocab_attn on bf16 rows: qkv16 [B*H*W][ldq] (ldq in ELEMENTS, a multiple of 8; base 16-byte aligned) holds head h of q / k / v
 * at q_off / k_off / v_off + 32 h (offsets multiples of 32): 30 channels followed by two exact zeros, q already multiplied by the
 * softmax scale.  The fp32 form rounds q * scale, k and v to bf16 on arrival, so on rows that hold those roundings the two forms agree
 * bit for bit. */
int ff_ocab_attn_rows16(const void* qkv16, int ldq, int q_off, int k_off, int v_off, float* out, int ldo, int o_off,
                        const float* rel_rotated, int B, int H, int W, int heads, int d, int ws, int ows, int out_bf16, void* stream);

/* DAT SGFN tail in one launch (plain bf16 MFMA, fp32 accumulate; dat_arch.py:117-123, 163-170, 736):
 *   out = res + W2 . ( h[:, :c2] * (dw3x3(LayerNorm(h[:, c2:2 c2])) + dw_bias) ) + b2
 * h rows [B*H*W][ldh >= 2 c2] (fc1's output), stats [tokens][2] = (mean, rstd) of h[:, c2:2 c2] (ff_token_linear stats_out), gamma /
 * beta [c2], dw_tapmajor [9][c2], fc2_tiles bf16 [hidden_tiles = ceil(c2/32)][192][32] (tile c, row n, column kk = W2[n][32 c + kk],
 * zero padded; prep.pack_sgfn_fc2), N <= 192 outputs.  The zero padding of the convolution applies to the NORMALISED tensor. */
int ff_sgfn_tail(const float* h, int ldh, int c2, const float* stats, const float* gamma, const float* beta,
                 const float* dw_tapmajor, const float* dw_bias, const void* fc2_tiles, int hidden_tiles, const float* b2,
                 const float* res, int ldr, float* out, int ldo, int B, int H, int W, int N, void* stream);

/* Depth-wise conv, NHWC, zero padding, weights tap-major [KH*KW][C]:
 *   out = act((sum w*x + bias) * post_scale + post_shift) * mul_in[pixel][c]     (mul_in may be NULL)
 * dat_arch.py:109,403-407; nafnet_arch.py:78-81; large_kernel_attention.py:59-73; edge_enhancement.py:62. */
int ff_dwconv2d(const float* in, int ldi, float* out, int ldo, int B, int H, int W, int C, int Ho, int Wo,
                const float* w_tapmajor, const float* bias, int KH, int KW, int sy, int sx, int py, int px,
                const float* post_scale, const float* post_shift, int act, const float* mul_in, int ldm, void* stream);

/* Depth-wise 3x3 / stride 1 / pad 1 with LayerNorm applied on load (csrc/dwconv.hip):
 *   out = (dw3x3( gamma * (in - mean[token]) * rstd[token] + beta ) + bias) * mul_in        zero padding AFTER the normalisation
 * stats [tokens][2] = (mean, rstd) per token from ff_token_linear's stats_out.  Replaces SpatialGate.forward's
 * norm + conv + gate product (dat_arch.py:117-123) without a separate LayerNorm pass. */
int ff_dwconv3x3_ln(const float* in, int ldi, float* out, int ldo, int B, int H, int W, int C, const float* w_tapmajor,
                    const float* bias, const float* stats, const float* gamma, const float* beta, const float* mul_in, int ldm,
                    void* stream);

/* out = ka*a*ca[c]*pa[p] + kb*b*cb[c]*pb[p]   (b, ca, cb, pa, pb may be NULL; clamp01 clamps to [0,1]) */
int ff_mix2(float* out, int ldo, const float* a, int lda, const float* b, int ldb, long long rows, int C, float ka,
            float kb, const float* ca, const float* cb, const float* pa, int ldpa, const float* pb, int ldpb,
            int clamp01, void* stream);
/* ff_mix2 with a channel scale per image: the rows are B equal groups of rows_per_image rows (rows == B * rows_per_image, the first
 * check) and ca is [B][C] (required): out = ka*a*ca[image][c]*pa[p] + kb*b*cb[c]*pb[p].  Every image has the bits of its own ff_mix2 call
 * with ca[b] (the cached-mode forward's collaborative gains [B][3] on the batch's expert outputs).  Added under ABI version 7 (additive). */
int ff_mix2_images(float* out, int ldo, const float* a, int lda, const float* b, int ldb, long long rows, int C, float ka,
                   float kb, const float* ca, int B, long long rows_per_image, const float* cb, const float* pa, int ldpa,
                   const float* pb, int ldpb, int clamp01, void* stream);
/* out = a + alpha*b*c   (a may be NULL) */
int ff_fma3(float* out, int ldo, const float* a, int lda, const float* b, int ldb, const float* c, int ldc,
            long long rows, int C, float alpha, void* stream);
/* out = act(in*scale[c] + shift[c])   (eval BatchNorm ahead of zero-padded convs) */
int ff_affine(float* out, int ldo, const float* in, int ldi, long long rows, int C, const float* scale,
              const float* shift, int act, void* stream);

/* Per-pixel two-layer MLP with a small hidden width and one output channel, fp32 (csrc/norm_pool.hip):
 *   out[p] = act2( w2 . act1( W1 x[p] + b1 ) + b2 ),   W1 [hidden][C] (hidden <= 16, C <= 192, C % 4 == 0), w2 [hidden].
 * Replaces the spatial-interaction branch of DAT's AdaptiveInteraction (dat_arch.py:585-590: conv1x1 + BN (folded) + GELU +
 * conv1x1 + sigmoid) in one pass over the token tensor. */
int ff_pixel_mlp(const float* in, int ldi, long long P, int C, int hidden, const float* W1, const float* b1, int act1,
                 const float* w2, float b2, int act2, float* out, void* stream);

/* Image I/O conversions of the plugin on the device (reference io.py:64-68 _load_image, :71-76 _save_image), so only uint8
 * crosses PCIe: in HWC uint8 [H][W][3] -> out fp32 [1][3][H][W] = v / 255 (IEEE division); and back: clamp to [0,1], * 255,
 * round half to even, uint8 HWC. */
int ff_u8hwc_to_f32nchw(const unsigned char* in, float* out, int H, int W, void* stream);
int ff_f32nchw_to_u8hwc(const float* in, unsigned char* out, int H, int W, void* stream);

/* NCHW image -> NHWC (+add[c]), padded to (Hp, Wp) with zeros (0) or reflection (1)
 * (expert_loader.py:63-96; nafnet_arch.py:220-225), and back (+add[c], crop, optional clamp to [0,1]). */
int ff_nchw_to_nhwc(const float* in, float* out, int B, int C, int H, int W, int Hp, int Wp, int ldo,
                    const float* add, int pad_mode, void* stream);
int ff_nhwc_to_nchw(const float* in, float* out, int B, int C, int H, int W, int Hs, int Ws, int ldi,
                    const float* add, int clamp01, void* stream);

/* Overlap-tile blending of the plugin's tiled fallback (models/team29_FreqFusion/io.py:104-121), planar NCHW:
 * acc[c][sy+y][sx+x] += tile[c][y][x]*wy[y]*wx[x]; wsum += wy*wx; then acc /= max(wsum, 1e-8). */
int ff_tile_accum(const float* tile, int C, int th, int tw, const float* wy, const float* wx, float* acc, float* wsum,
                  int H, int W, int sy, int sx, void* stream);
int ff_tile_normalize(float* acc, const float* wsum, int C, int H, int W, void* stream);

/* The image side of the tiled executor (csrc/tile_image.hip; ff_forward_image_u8 below drives them, each is usable alone).
 *   ff_tile_positions  pure host, no GPU call: the tile origins along an axis of n samples (io.py:87-91) --
 *                      range(0, max(n - tile + 1, 1), step), plus n - tile when the last tile stops short of the border -- into
 *                      out[0..count); returns the count, or -1 for n < tile, step < 1, tile < 1, a null out or count > cap.
 *   ff_tile_cut_u8     img uint8 HWC [H][W][3] -> out fp32 planar [3][th][tw], the tile at (y, x): u8 / 255 by IEEE division, the
 *                      bits of ff_u8hwc_to_f32nchw followed by a slice copy.  The tile must lie inside the image.
 *   ff_tile_ramps      tab [4][st], the edge weights of io.py:97-113: row v is ones; with bit 0 of v the first `blend` samples are
 *                      ramp = np.linspace(0, 1, blend, dtype=float32), with bit 1 the last `blend` are 1 - ramp (fp32).  blend 0
 *                      gives ones, blend 1 the ramp [0]; 0 <= blend <= st.
 *   ff_tile_finish_u8  acc [3][H][W], wsum [H][W] (the un-normalised canvas, only read) -> out uint8 HWC [H][W][3]:
 *                      acc / max(wsum, 1e-8), clamp to [0,1], * 255, round half to even -- the bytes of ff_tile_normalize
 *                      followed by ff_f32nchw_to_u8hwc, in one pass.  Four pixels per thread when out is 4-byte aligned. */
int ff_tile_positions(int n, int tile, int step, int* out, int cap);
int ff_tile_cut_u8(const unsigned char* img, int H, int W, int y, int x, int th, int tw, float* out, void* stream);
int ff_tile_ramps(float* tab, int st, int blend, void* stream);
int ff_tile_finish_u8(const float* acc, const float* wsum, int H, int W, unsigned char* out, void* stream);

/* The two kernels of the tiled executor's x8 self-ensemble (csrc/tile_image.hip; ff_forward_image_ens_u8 below drives them, each is
 * usable alone).  `code` (0..15, a HOST int) has ff_d4_nchw's meaning and order: bit 0 flip(-1), then bit 1 flip(-2), then
 * rot90(k = code >> 2, dims (-2, -1)).  Both added under ABI version 7 (additive entry points: no existing prototype changed).
 *   ff_tile_cut_u8_d4  the tile at (y, x) of the TRANSFORMED image T_code(img), which is never materialised: img uint8 HWC [H][W][3]
 *                      -> out fp32 planar [3][th][tw].  T_code(img) is H x W for even k and W x H for odd k; the tile must lie inside
 *                      THAT shape.  The bits of ff_d4_rect_nchw(ff_u8hwc_to_f32nchw(img), code)[..., y:y+th, x:x+tw]: u8 / 255 by
 *                      IEEE division, then the permutation.  One pixel per thread, the fp32 stores coalesced for every code.
 *   ff_tile_fold_d4    acc [3][Hc][Wc], wsum [Hc][Wc] (one variant's un-normalised canvas, only read) folded into ens [3][Hd][Wd],
 *                      (Hd, Wd) = (Hc, Wc) for even k and (Wc, Hc) for odd k.  With v = acc / max(wsum, 1e-8) (ff_tile_normalize's
 *                      arithmetic, one rounding) and t = T_code(v):  accum 0: ens = t * scale;  accum 1: ens = (ens + t) * scale,
 *                      the add rounded first, then the multiply, no contraction -- the bits of ff_tile_normalize on a copy of acc
 *                      followed by ff_d4_rect_nchw(..., code, accum, scale), in one pass (40 instead of 64 bytes per pixel).  No
 *                      atomics; ens may overlap neither acc nor wsum. */
int ff_tile_cut_u8_d4(const unsigned char* img, int H, int W, int code, int y, int x, int th, int tw, float* out, void* stream);
int ff_tile_fold_d4(const float* acc, const float* wsum, int Hc, int Wc, int code, float* ens, int accum, float scale, void* stream);

/* Bilinear (mode 0) / bicubic A=-0.75 (mode 1) resize, align_corners=False, generic element strides.
 * scale_* = source step per destination pixel exactly as ATen computes it. */
int ff_resize(const float* in, long long isb, long long isc, long long isy, long long isx, int Hi, int Wi, float* out,
              long long osb, long long osc, long long osy, long long osx, int Ho, int Wo, int B, int C, float scale_h,
              float scale_w, int mode, float mul, void* stream);
int ff_avgpool2(const float* in, int ldi, float* out, int ldo, int B, int H, int W, int C, void* stream);

/* Device half of the cached-expert data-set builder (isr2_amd.cache.build_from_folders; csrc/resample.hip).  The reference's reader
 * (src/data/cached_dataset.py:45-50) expects "several crops per image" files that nothing in its tree writes; its pairing rules are
 * PairedRandomCrop (augmentations.py:77-83) and the centre crop of dataset.py:282-296.
 * ff_crop_pairs_u8: K aligned patch pairs out of uploaded uint8 images in one launch.  lr_u8 [h][w][3], hr_u8 [4h][4w][3] (HWC), pos =
 *   DEVICE int32 [K][2] of LR (top, left) with 0 <= top <= h - p, 0 <= left <= w - p (the caller checks them: ops.crop_pairs_u8);
 *   lr_out [K][3][p][p], hr_out [K][3][4p][4p] fp32 = u8 / 255 (IEEE division, as ff_u8hwc_to_f32nchw); HR patch k starts at
 *   (4 top, 4 left).
 * ff_resize_aa: antialiased bicubic x1/4 of planar fp32 [planes][Hi][Wi] -> [planes][Ho][Wo], Hi = 4 Ho, Wi = 4 Wo -- F.interpolate(
 *   mode='bicubic', antialias=True, align_corners=False), cubic a = -0.5 stretched by the scale.  Separable, horizontal pass first; per
 *   axis a DEVICE table from ops.aa_tables: span [O][2] int32 = (first input index, number of taps <= 16), wt [O][16] fp32 = normalised
 *   weights, zero padded (16-byte aligned).  Each pass: acc = fma(w_j, x[first + j], acc) from 0, ascending j.
 * Both added under ABI version 7 (additive entry points: no existing prototype changed). */
int ff_crop_pairs_u8(const unsigned char* lr_u8, const unsigned char* hr_u8, int h, int w, const int* pos, int K, int p, float* lr_out,
                     float* hr_out, void* stream);
int ff_resize_aa(const float* in, float* out, int planes, int Hi, int Wi, int Ho, int Wo, const int* span_w, const float* wt_w,
                 const int* span_h, const float* wt_h, void* stream);
/* OpenCV's INTER_CUBIC restated (cv2.resize in the reference's ValidationDataset, dataset.py:473-506; csrc/resample.hip,
 * ops.resize_cv_cubic, epoch.live_val_images): planar fp32 [planes][Hi][Wi] -> [planes][Ho][Wo] at any ratio, up or down; four taps per
 * axis whatever the ratio (no antialiasing), replicated border, no clamping of values.  Per axis a DEVICE table from
 * ops.cv_cubic_tables: idx [O][4] int32 = taps s - 1 .. s + 2 clamped to [0, n_in - 1], wt [O][4] fp32 = interpolateCubic's weights
 * (A = -0.75f) of x = f - s, f = float((d + 0.5) * (double(n_in) / n_out) - 0.5), s = floor(f).  Per source row
 * h = ((v0 a0 + v1 a1) + v2 a2) + v3 a3 with the horizontal weights, then out = ((h0 b0 + h1 b1) + h2 b2) + h3 b3 with the vertical ones,
 * every product and sum rounded on its own (no fused multiply-add).  The kernel clamps the table indices again, so no table reads outside
 * the image.  First check, before any launch: null pointers, a size < 1, a size > 2^20, the grid bound.  Added under ABI version 7 (an
 * additive entry point: no existing prototype changed). */
int ff_resize_cv_cubic(const float* in, float* out, int planes, int Hi, int Wi, int Ho, int Wo, const int* idx_w, const float* wt_w,
                       const int* idx_h, const float* wt_h, void* stream);

/* One training micro-batch out of a resident image pool (isr2_amd.epoch.ImagePool / LiveEpoch; csrc/sample_batch.hip): crop, u8 -> fp32
 * and the paired D4 augmentation of B samples, LR and HR, in one launch.  pool: one device byte buffer, every image uint8 HWC packed
 * back to back (nothing aligned).  desc: DEVICE int64 [B][8] = {lr_off, hr_off, h, w, top, left, code, 0} -- byte offsets into pool, LR
 * image [h][w][3], HR partner [4h][4w][3], LR patch origin with 0 <= top <= h - p, 0 <= left <= w - p, code as ff_d4_nchw (bit 0
 * flip(-1), bit 1 flip(-2), bits 2-3 rot90 k); the caller checks them (ops.sample_pairs_u8), the kernel clamps top / left all the same.
 * lr_out [B][3][p][p], hr_out [B][3][4p][4p] fp32 = u8 / 255 (IEEE division): the bits of ff_d4_nchw(ff_crop_pairs_u8(...)).
 * First check: null pointers, B < 1, p < 1.  Added under ABI version 7 (additive). */
int ff_sample_pairs_u8(const unsigned char* pool, const long long* desc, int B, int p, float* lr_out, float* hr_out, void* stream);

/* One cached-expert micro-batch out of a resident sample pool (isr2_amd.epoch.ResidentCache / ResidentEpoch; csrc/gather_batch.hip): the
 * B samples desc names, every field of them, gathered and D4-augmented in one launch.  pool: one device fp32 buffer, FIELD-major --
 * field f is a contiguous [n_samples][C_f][H_f][W_f] array that starts fields[f][0] floats into pool.  fields: HOST int64 [F][5] =
 * {pool_off, out_off, C, H, W}, 1 <= F <= 8, read before the launch (as codes is in ff_forward_image_ens_u8).  desc: DEVICE int32
 * [B][2] = {sample index, code}, code as ff_d4_nchw (bit 0 flip(-1), bit 1 flip(-2), bits 2-3 rot90 k).  out: flat; field f of the
 * micro-batch is [B][C_f][H_f][W_f] starting at out + fields[f][1] = the bits of ff_d4_nchw(field_f[index], codes).  A pure copy: NaN
 * payloads, -0 and denormals pass through.  The 16-byte form is chosen per field (W_f % 4 == 0 and both of its bases 16-byte aligned),
 * the dword form otherwise.  The caller checks indices and codes (ops.gather_d4_fields); the kernel clamps the index into
 * [0, n_samples), masks the code to 4 bits and clears its odd-turn bit on a non-square field all the same, so no descriptor reads outside
 * the pool.  First check, before any launch: null pointers, B < 1, F outside 1..8, n_samples < 1, a non-positive dimension, a negative
 * offset, 2^31 tiles or more.  Added under ABI version 7 (an additive entry point: no existing prototype changed). */
int ff_gather_d4_fields(const float* pool, long long n_samples, const long long* fields, int F, const int* desc, int B, float* out,
                        void* stream);

/* The reference's paired colour jitter (augmentations.py:207-264) on a sampled micro-batch, in place (csrc/color_jitter.hip;
 * ops.color_jitter_pairs, epoch.LiveEpoch(color_jitter=...)).  lr [B][3][p][p], hr [B][3][4p][4p] fp32 = u / 255 as ff_sample_pairs_u8 writes
 * them; table: DEVICE fp32 [B][4] = {apply, bf, cf, sf} -- apply == 0 leaves both patches of that sample untouched bit for bit.  Per patch
 * (each with its OWN mean): mean = float(double(bf) * (double(S) / (255.0 * 3 P P))) with S the exact integer sum of the patch's bytes
 * rint(255 x); x2 = (x * bf - mean) * cf + mean, every fp32 step rounded on its own (no fused multiply-add); sf == 1: out = clip(x2, 0, 1);
 * otherwise q = (u8) trunc(255 clip(x2)), 8-bit RGB -> HSV (12-bit fixed point, H in 0..179), S' = (u8) trunc(clip(S * sf, 0, 255)), HSV ->
 * RGB (fp32 sector table, bytes by rint), out = byte / 255.  Two launches: the integer sums (64-bit partials in the workspace, no atomics),
 * then the per-pixel pass.  workspace: ff_color_jitter_workspace(B) BYTES (-1 for B < 1), 8-byte aligned, need not be zeroed.
 * First check: null pointers, B < 1, p < 1; then p <= 8192, B <= 2^20, the workspace size, the grid bound.  Added under ABI version 7
 * (additive). */
long long ff_color_jitter_workspace(int B);
int ff_color_jitter_pairs(float* lr, float* hr, const float* table, int B, int p, void* workspace, long long workspace_bytes, void* stream);

/* Frequency bands of the planar LR image x[C][H][W] written into out[H][W][ldo] channel groups.
 * multi_domain_frequency.py:146-196 (DCT), :273-299 (DWT pass), :352-385 (FFT low/high). */
int ff_dct8_bands(const float* x, int C, int H, int W, const float* dct_mat, const float* masks3,
                  const float* band_scale, float* out, int ldo, int ch_off, void* stream);
int ff_dwt_pass(const float* in, int C, int H, int W, int axis, const float* lo8, const float* hi8, float* out_lo,
                float* out_hi, void* stream);
int ff_fft_bands(const float* x, int C, int H, int W, const float* twW_cos, const float* twW_sin,
                 const float* twH_cos, const float* twH_sin, const float* mask_logits, int msz, float temp,
                 const float* band_scale2, float* work, long long work_floats, float* out, int ldo, int ch_lo,
                 int ch_hi, void* stream);
/* The DCT and FFT bands of B images in one launch each (one run of the four FFT kernels): x [B][3][H][W] -> out [B][H][W][ldo], the
 * channel groups of ff_dct8_bands (ch_off .. ch_off + 8) / ff_fft_bands (ch_lo .. + 2, ch_hi .. + 2) in every image, each image with the
 * bits of its own single-image call.  First check of both: 1 <= B, 3 B <= 65535 (the planes index gridDim.y of the FFT's column passes),
 * H, W >= 8 (DCT) / H, W > 1, W <= 8192 and an H whose column tile fits 64 KiB of LDS as in ff_fft_bands (H <= 481 or 513 <= H <= 1638) (FFT); then null pointers, the workspace and ldo >= the channels written.
 * The FFT's column passes take their decomposition (columns per workgroup, output-row split) from ONE image's three planes.
 * work: ff_fft_bands_images_workspace(B, H, W) floats = B x the 4 * 3 * H * (W / 2 + 1) of one image (-1 for a refused geometry).
 * Added under ABI version 7 (additive). */
int ff_dct8_bands_images(const float* x, int B, int H, int W, const float* dct_mat, const float* masks3,
                         const float* band_scale, float* out, int ldo, int ch_off, void* stream);
long long ff_fft_bands_images_workspace(int B, int H, int W);
int ff_fft_bands_images(const float* x, int B, int H, int W, const float* twW_cos, const float* twW_sin,
                        const float* twH_cos, const float* twH_sin, const float* mask_logits, int msz, float temp,
                        const float* band_scale2, float* work, long long work_floats, float* out, int ldo, int ch_lo,
                        int ch_hi, void* stream);

/* DAT channel attention (dat_arch.py:627-647): token-axis L2 norms + per-head 30x30 gram + softmax ->
 * block-diagonal [180][180] matrix (apply with ff_conv2d on v).  work: ff_chan_attn_workspace floats. */
int ff_chan_attn_weights(const float* qkv, int ld, int q_off, int k_off, long long N, const float* temperature,
                         float* wbd, float* work, long long work_floats, void* stream);
long long ff_chan_attn_workspace(long long N);

/* DAT channel attention, fused front end (csrc/chan_qkv.hip; dat_arch.py:617-641): LayerNorm + qkv projection + per-head gram
 * q_h^T k_h and squared column norms over all tokens in ONE launch -- q and k never reach memory; v [M][ldv] is written for the
 * depth-wise branch and the attention product.  w_tiles: bf16 [18][2][32][192] = q_0, k_0, ..., q_5, k_5 (head dim padded to 32
 * rows) then v rows 0..191 in six tiles (prep.pack_chan_qkv); work: ff_chan_qkv_workspace(M) floats, afterwards holding one
 * 5760-float partial per 256 tokens.  ff_chan_attn_finish reduces them, L2-normalises, applies the temperature and the softmax and
 * emits the block-diagonal [180][180] matrix of ff_chan_attn_weights (nblk = ceil(M / 256)). */
long long ff_chan_qkv_workspace(long long M);
int ff_chan_qkv(const float* x, int ldx, long long M, int K, const float* gamma, const float* beta, float eps, const void* w_tiles,
                const float* bias_padded, float* v_out, int ldv, float* work, long long work_floats, int nterms, void* stream);
int ff_chan_attn_finish(float* work, long long work_floats, int nblk, const float* temperature, float* wbd, void* stream);
/* B images: ONE ff_chan_qkv call on all B * rows_per_image rows (rows_per_image % 256 == 0, so every 256-token partial is one image's)
 * leaves partials [B][nblk][5760] in work; ff_chan_attn_finish_images reduces image b's nblk = rows_per_image / 256 blocks in the
 * single-image order (G [B][5760] follows the partials) and emits wbd [B][180][180].  work: ff_chan_qkv_images_workspace floats = B times
 * one image's (-1 for a refused geometry).  Added under ABI version 7 (additive). */
long long ff_chan_qkv_images_workspace(int B, long long rows_per_image);
int ff_chan_attn_finish_images(float* work, long long work_floats, int B, long long rows_per_image, const float* temperature, float* wbd,
                               void* stream);

/* Fusion-stack pointwise kernels (see csrc/fusion_ops.hip for the reference lines). */
int ff_band_mha_core(const float* qkv, float* out, long long P, int nbands, int heads, void* stream);
int ff_band_weight(const float* x, const float* att, const float* imp, float* out, long long P, int nbands,
                   void* stream);
int ff_freq_guidance(const float* bands3, float* guide, long long P, void* stream);
int ff_dynamic_gates(const float* graw, const float* dif, float* gates, long long P, void* stream);
int ff_fuse_blend(const float* experts9, const float* hier3, const float* guide3, const float* gates3,
                  const float* dif1, float* out3, int Hh, int Wh, int Hl, int Wl, void* stream);
/* ff_fuse_blend for B images in one launch (grid: one image's blocks x B): contiguous [B][...] tensors, image b's experts9 / hier3 / out3
 * at b * Hh * Wh * {9, 3, 3} and guide3 / gates3 / dif1 at b * Hl * Wl * {3, 3, 1}.  First check: 1 <= B <= 65535 and positive sizes.
 * Added under ABI version 7 (additive). */
int ff_fuse_blend_images(const float* experts9, const float* hier3, const float* guide3, const float* gates3,
                         const float* dif1, float* out3, int B, int Hh, int Wh, int Hl, int Wl, void* stream);

/* Device PSNR / SSIM evaluator (csrc/metrics.hip; reference src/utils/metrics.py:30-52 rgb_to_y, :76-126 calculate_psnr,
 * :129-190 calculate_ssim_torch).  a, b: planar fp32 images [C][H][W], C = 1 or 3; values are clamped to [0,1], `crop` border
 * pixels are dropped, use_y != 0 converts RGB to BT.601 luma first.  work: ff_metric_workspace(C,H,W,crop) doubles.
 * ff_psnr_mse writes the mean squared error, ff_ssim_mean the mean of the SSIM map (11-tap separable Gaussian gauss11,
 * zero padding) to a device double; both are deterministic (fixed-order double-precision reduction). */
int ff_metric_workspace(int C, int H, int W, int crop);
int ff_psnr_mse(const float* a, const float* b, int C, int H, int W, int crop, int use_y, double* work, int nwork, double* out_mse,
                void* stream);
int ff_ssim_mean(const float* a, const float* b, int C, int H, int W, int crop, int use_y, const float* gauss11, double* work,
                 int nwork, double* out_ssim, void* stream);

/* ------------------------------------------------------------------------------------------------------------------------
 * Training side (csrc/train_ops.hip): the backward halves and the optimizer of the fusion-only training step -- BASELINE config 5,
 * SURVEY 8f rank 1.  Replaces what autograd + torch.optim do in the reference's train.py:308-356 (`train_epoch_cached`: forward_with_
 * precomputed -> clamp -> L1 -> backward -> clip_grad_norm_(1.0) -> AdamW.step -> EMA.update).  All fp32, all reductions two-stage in a
 * fixed order (bit-reproducible steps).  Tensors are dense rows [rows][ld]; `accumulate` != 0 adds into the destination.
 *
 * Broadcast operands (ff_ew_fma): kind 0 = full [rows][ld], 1 = one value per row (element r*ld), 2 = one value per (row group,
 * column) [rows / rows_per_group][C], 3 = ONE device scalar (learnable scalars such as LKABlock.scale1, residual_scale,
 * edge_strength stay on the device), 4 = absent. */
int ff_ew_fma(float* out, int ldo, const float* a, int lda, const float* b, int ldb, int b_kind, const float* c, int ldc, int c_kind,
              float c_scale, long long rows, int C, long long rows_per_group, int clamp01, void* stream);
/* out = f(x) for op < 16, out = g * f'(x) for op >= 16:
 *   0 GELU (erf) 1 ReLU 2 sigmoid 3 softplus 4 abs 5 clamp01 6 x*p0 7 1/(x+p0) 8 max(x,p0) 9 exp
 *   16 GELU' 17 ReLU' 18 sigmoid' from the OUTPUT y 19 softplus' 20 abs' (sgn, 0 at 0) 21 clamp01' (bounds inclusive, as torch.clamp)
 *   22 d(1/(u+eps)) from the output y: -g y^2   23 clamp_min' (x >= p0)   24 exp' from the output y */
int ff_ew_unary(int op, const float* x, int ldx, const float* g, int ldg, float* out, int ldo, long long rows, int C, float p0,
                void* stream);
/* out[g][c] = scale * sum_{r in group g} x[r][c] * (y[r][c] | y[r*ldy] | 1): bias / BatchNorm / per-channel-scale gradients.
 * y_kind 0 full, 1 per row, 4 absent. */
long long ff_reduce_cols_workspace(long long rows, int C, long long rows_per_group);
int ff_reduce_cols(const float* x, int ldx, const float* y, int ldy, int y_kind, long long rows, int C, long long rows_per_group,
                   float scale, float* out, int accumulate, float* work, long long work_floats, void* stream);
/* out[r*ldo] = scale * sum_c x[r][c] * (y[r][c] | y[c] | 1): per-pixel gate gradients.  y_kind 0 full, 2 per column, 4 absent. */
int ff_reduce_rows(const float* x, int ldx, const float* y, int ldy, int y_kind, long long rows, int C, float scale, float* out,
                   int ldo, int accumulate, void* stream);

/* Weight gradient of nn.Conv2d (stride 1, 'same' padding) / nn.Linear on the fp32 matrix cores:
 *   dw[co][(ky*KW + kx)*Cin + ci] = sum_{b,y,x} dz[b,y,x,co] * in[b, y+ky-py, x+kx-px, ci]      (same packed layout as ff_conv2d's w)
 * The data gradient is ff_conv2d of dz with ff_conv_weight_flipT(w): wt[ci][flipped tap][co]. */
long long ff_conv2d_wgrad_workspace(int B, int H, int W, int Cin, int Cout, int KH, int KW);
int ff_conv2d_wgrad(const float* in, int ldx, const float* dz, int ldz, float* dw, int B, int H, int W, int Cin, int Cout, int KH,
                    int KW, int py, int px, int accumulate, float* work, long long work_floats, void* stream);
int ff_conv_weight_flipT(const float* w, float* wt, int Cout, int Cin, int KH, int KW, void* stream);
/* Depth-wise convolutions of the LKA chain (large_kernel_attention.py:59-73: 5x5, 1x21, 21x1) and 3x3: weight gradient in the
 * tap-major layout [KH*KW][C] of ff_dwconv2d; the data gradient is ff_dwconv2d with ff_taps_reverse(w). */
long long ff_dwconv2d_wgrad_workspace(int B, int H, int W, int C, int KH, int KW);
int ff_dwconv2d_wgrad(const float* in, int ldx, const float* dy, int ldy, float* dw, int B, int H, int W, int C, int KH, int KW,
                      int accumulate, float* work, long long work_floats, void* stream);
int ff_taps_reverse(const float* w, float* out, int taps, int C, void* stream);
/* Adjoints of F.interpolate(mode='bilinear', align_corners=False) (NHWC; scale_* as ff_resize) and F.avg_pool2d(2). */
int ff_resize_bilinear_adj(const float* dy, int ldy, int Ho, int Wo, float* dx, int ldx, int Hi, int Wi, int B, int C, float scale_h,
                           float scale_w, float mul, int accumulate, void* stream);
int ff_avgpool2_adj(const float* dy, int ldy, float* dx, int ldx, int B, int H, int W, int C, int accumulate, void* stream);
/* nn.LayerNorm backward: dx, and dgamma_dbeta [2][C] = (sum dy*xhat, sum dy).  C <= 256. */
long long ff_layernorm_bwd_workspace(long long rows, int C);
int ff_layernorm_bwd(const float* x, int ldx, const float* dy, int ldy, const float* gamma, float eps, float* dx, int lddx,
                     long long rows, int C, float* dgamma_dbeta, int accumulate, float* work, long long work_floats, void* stream);
/* nn.BatchNorm2d in TRAINING mode (LKABlock.norm1 / lka.bn / norm2, MultiScaleFeatureExtractor's BatchNorms): G calls (one per band /
 * expert / scale) of `count` pixels each.  finish: mean_rstd [G][C][2], scale = gamma*rstd and shift = beta - mean*scale [G][C]
 * (apply with ff_ew_fma kinds 2), running statistics updated call by call with `momentum` and the unbiased variance.
 * bwd: dx from sum_dy / sum_dy_xhat [G][C] (ff_reduce_cols of dy and of dy * ff_bn_xhat). */
int ff_bn_train_finish(const float* sum_x, const float* sum_x2, int centered, int G, int C, long long count, const float* gamma,
                       const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean_rstd,
                       float* scale, float* shift, void* stream);
int ff_bn_xhat(const float* x, int ldx, const float* mean_rstd, float* out, int ldo, long long rows, int C, long long rows_per_group,
               void* stream);
int ff_bn_train_bwd(const float* x, int ldx, const float* dy, int ldy, const float* mean_rstd, const float* gamma, const float* sum_dy,
                    const float* sum_dy_xhat, float* dx, int lddx, long long rows, int C, long long rows_per_group, void* stream);
/* ff_band_mha_core with dropout on the attention weights (nn.MultiheadAttention(dropout=0.1) in training mode,
 * large_kernel_attention.py:196,296; counter-based mask from `seed`) and its backward (dqkv rows [(p*ntok + i)][3E]). */
int ff_band_mha_train(const float* qkv, float* out, long long P, int ntok, int heads, float drop_p, unsigned long long seed,
                      void* stream);
long long ff_band_mha_bwd_workspace(long long P, int ntok, int heads);
int ff_band_mha_bwd(const float* qkv, const float* dout, float* dqkv, long long P, int ntok, int heads, float drop_p,
                    unsigned long long seed, float* work, long long work_floats, void* stream);
int ff_dynamic_gates_bwd(const float* graw, const float* dif, const float* dgates, float* dgraw, float* ddif, long long P, void* stream);
/* [A][B][C] -> [B][A][C] (tokens (pixel, band) <-> band-major images) */
int ff_permute_rows(const float* in, float* out, long long A, long long Bd, int C, void* stream);
/* rfft2 / irfft2 (norm='ortho') of planar images, spectra [planes][H][W/2+1][2] (csrc/freq.hip); the learnable mask between them
 * (multi_domain_frequency.py:362-385): Y = X*m, and dm = sum_planes Re(gY conj X) with torch's c2r column doubling. */
int ff_rfft2(const float* x, int C, int H, int W, const float* twW_cos, const float* twW_sin, const float* twH_cos,
             const float* twH_sin, float* work, long long work_floats, float* spec, void* stream);
int ff_irfft2(const float* spec, int C, int H, int W, const float* twW_cos, const float* twW_sin, const float* twH_cos,
              const float* twH_sin, float* work, long long work_floats, float* out, void* stream);
int ff_spec_mask_mul(const float* X, const float* m, float* Y, int planes, int H, int Wf, void* stream);
int ff_spec_mask_grad(const float* gY, const float* X, float* dm, int planes, int H, int W, int accumulate, void* stream);
/* loss = mean |clamp(sr,0,1) - hr| and its gradient (train.py:318-321 with the stage-1 weights l1 = 1, perceptual_loss.py:86-105);
 * total squared gradient norm; clip_grad_norm_ + torch.optim.AdamW + EMAModel.update (train.py:338-351, checkpoint_manager.py:400-407)
 * over one flat buffer.  hyper10 (device): lr, beta1, beta2, eps, weight_decay, max_norm (<= 0: off), ema_decay, step,
 * lr / (1 - beta1^step), sqrt(1 - beta2^step).  work: 1024 floats. */
int ff_l1_loss_grad(const float* sr, const float* hr, float* dsr, long long n, float* loss, float* work, long long work_floats,
                    void* stream);
int ff_grad_sqnorm(const float* g, long long n, float* out_sqnorm, float* work, long long work_floats, void* stream);
int ff_adamw_ema_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, float* ema, long long n, const float* hyper10,
                      const float* sqnorm, void* stream);

/* The reference's staged training losses (csrc/sr_losses.hip; CombinedLoss, perceptual_loss.py:1207-1283).  sr (pre-clamp) and hr
 * are NHWC [B][H][W][3]; each component writes its UNWEIGHTED value to value[0] (device) and, when dsr is not null, stores
 * (accumulate = 0) or adds (accumulate = 1) weight * d(value)/d(sr) with the clamp mask 0 <= sr <= 1.  Fixed-order reductions:
 * identical calls give identical bits.  Workspace in floats: ff_loss_workspace(component, B, H, W), component 0 l1, 1 charbonnier,
 * 2 l2, 3 ssim, 4 edge, 5 swt, 6 fft.
 *   ff_loss_pointwise  kind 0 l1, 1 charbonnier (eps 1e-6), 2 l2
 *   ff_loss_ssim       1 - mean SSIM (gauss11: the normalised 11-tap Gaussian, sigma 1.5; zero padding 5; C1 0.01^2, C2 0.03^2)
 *   ff_loss_edge       l1(Sobel x) + l1(Sobel y), zero padding 1
 *   ff_loss_swt        SWTLoss('haar', 2, use_gpu_approximation=True); band weights a 0.5, h 1.5, v 1.5, d 2.0
 *   ff_loss_fft        FFTLoss(focus_high_freq=True); tw*: the twiddle tables of ff_rfft2
 *   ff_loss_combine    total[0] = sum_k weights[k] * values[k] (device arrays), added in order */
long long ff_loss_workspace(int component, int B, int H, int W);
int ff_loss_pointwise(int kind, const float* sr, const float* hr, int B, int H, int W, float weight, float* dsr, int accumulate,
                      float* value, float* work, long long work_floats, void* stream);
int ff_loss_ssim(const float* sr, const float* hr, int B, int H, int W, const float* gauss11, float weight, float* dsr, int accumulate,
                 float* value, float* work, long long work_floats, void* stream);
int ff_loss_edge(const float* sr, const float* hr, int B, int H, int W, float weight, float* dsr, int accumulate, float* value,
                 float* work, long long work_floats, void* stream);
int ff_loss_swt(const float* sr, const float* hr, int B, int H, int W, float weight, float* dsr, int accumulate, float* value,
                float* work, long long work_floats, void* stream);
int ff_loss_fft(const float* sr, const float* hr, int B, int H, int W, const float* twW_cos, const float* twW_sin, const float* twH_cos,
                const float* twH_sin, float weight, float* dsr, int accumulate, float* value, float* work, long long work_floats,
                void* stream);
int ff_loss_combine(const float* values, const float* weights, int k, float* total, void* stream);

/* Paired training augmentation (csrc/augment.hip; CachedSRDataset._apply_augmentation, src/data/cached_dataset.py:240-268): every
 * sample b of a planar batch in [B][C][H][W] -> out [B][C][H][W] takes its own symmetry of the square, codes[b] (DEVICE ints) =
 * bit 0 hflip | bit 1 vflip | bits 2-3 k, applied in the reference's order flip(-1), flip(-2), rot90(k, dims (-2, -1)).  Odd k
 * transposes, so it needs H == W (on a non-square batch the bit is ignored: the host wrapper refuses such codes before any launch).
 * A pure permutation, not in place; one launch per tensor per batch. */
int ff_d4_nchw(const float* in, float* out, int B, int C, int H, int W, const int* codes, void* stream);

/* One symmetry of the square on RECTANGULAR planes, with fused accumulation (csrc/augment.hip; the building block of the x8 geometric
 * self-ensemble, isr2_amd.model.FreqFusionHIP.self_ensemble).  src [B][C][Hs][Ws] -> dst [B][C][Hd][Wd], both contiguous, with
 * (Hd, Wd) = (Hs, Ws) when k = code >> 2 is even and (Ws, Hs) when it is odd; any Hs, Ws >= 1.  `code` (0..15, a HOST int, one for the
 * whole launch) has ff_d4_nchw's meaning and order: bit 0 flip(-1), then bit 1 flip(-2), then rot90(k, dims (-2, -1)).  With t the
 * transformed plane:  accum 0: dst = t * scale;  accum 1: dst = (dst + t) * scale -- the add is rounded first, then the multiply, no
 * contraction (scale = 1 leaves the sum's bits untouched).  No atomics; not in place (src != dst). */
int ff_d4_rect_nchw(const float* src, float* dst, int B, int C, int Hs, int Ws, int code, int accum, float scale, void* stream);

/* C-level executor (csrc/ff_executor.hip): the whole forward -- models/team29_FreqFusion/io.py:221 `model(lr)` =
 * CompleteEnhancedFusionSR.forward, src/models/enhanced_fusion.py:694-754 -- for callers without Python.  A plan
 * (<stem>.ffplan, written by isr2_amd.plan.export_plan) lists every launch of one input shape with pointers expressed as
 * (prepared-weight slot | workspace | input | output, offset); <stem>.ffwts carries the prepared weights.
 *   ff_create    load a plan on the CURRENT device; allocates the weight slots and the workspace (the library owns both)
 *   ff_upload    copy `nbytes` from a host or device buffer into the named slot (sizes must match the plan)
 *   ff_finalize  succeeds once every slot has been uploaded
 *   ff_forward   lr_dev [B,3,H,W] fp32 -> out_dev [B,3,4H,4W]; all launches go to `stream` in plan order (asynchronous,
 *                graph-capturable); B, H, W must be the plan's
 *   ff_destroy   frees everything the handle owns
 * Handles are not thread-safe; use one per host thread (kernels of different handles may run on different streams).
 *
 * Images of ANY size through one TILE plan (a plan exported on [B,3,t,t] -> [B,3,4t,4t], square tiles, B <= 16): the plugin's
 * overlap-tile path (models/team29_FreqFusion/io.py:116-164, _tiled_forward) with its exact result, B tiles per replay, uint8 in and out.
 *   ff_image_workspace_bytes  the size of `work` for an H x W image; -1 (and a message) for a null handle, a plan that is no tile
 *                             plan, or an image smaller than the tile
 *   ff_forward_image_u8       img_dev uint8 HWC [H][W][3] -> out_dev uint8 HWC [4H][4W][3], tiles of step t - overlap blended with
 *                             linear ramps of min(4 overlap, t) samples.  Needs a finalized handle, H >= t and W >= t (every tile
 *                             is then full-size; ragged tiles are out of scope), 0 <= overlap < t, work_bytes >= the size above;
 *                             all of it is checked before the first launch.  Everything runs on `stream`: no allocation, no host
 *                             synchronisation, no host-to-device copy -- asynchronous and graph-capturable like ff_forward.
 * `work` is the caller's device buffer; its parts, each starting on a multiple of 256 bytes, in this order (fp32):
 *     acc [3][4H][4W] | wsum [4H][4W] | tile input [B,3,t,t] | tile output [B,3,4t,4t] | ramp table [4][4t]
 * acc and wsum hold the un-normalised canvas when the call has run (ff_tile_normalize(acc, wsum) gives the fp32 image).
 *
 * The x8 geometric self-ensemble of such an image (isr2_amd.model.FreqFusionHIP.self_ensemble with the tiled forward as `run`), added
 * under ABI version 7:
 *   ff_image_ens_workspace_bytes  the size of `work` for the ensemble of an H x W image; -1 (and a message) in the cases of
 *                                 ff_image_workspace_bytes
 *   ff_forward_image_ens_u8       img_dev uint8 HWC [H][W][3] -> out_dev uint8 HWC [4H][4W][3], the average of the model's outputs over
 *                                 the symmetries codes[0..ncodes) -- a HOST array of ff_d4_nchw codes (0..15), no symmetry named twice
 *                                 (codes 8..15 repeat 0..7); 0..7 is the x8 ensemble.  Per code, in the order given: the canvas of
 *                                 T_code(img) from its tiles exactly as ff_forward_image_u8 builds the plain one (an odd quarter turn
 *                                 makes it W x H; tiles come from ff_tile_cut_u8_d4), then one ff_tile_fold_d4 with the inverse code,
 *                                 accum = (i > 0) and scale = 1, the last one scale = (float)(1.0 / ncodes); at the end
 *                                 ff_f32nchw_to_u8hwc(ens).  Same requirements and guarantees as ff_forward_image_u8 (H >= t and
 *                                 W >= t cover both orientations), all checked before the first launch.
 * Its `work`: the parts of ff_forward_image_u8 for an H x W image, in the same order (a W x H canvas has the same element count),
 * followed by ens [3][4H][4W] fp32, which starts on a multiple of 256 bytes and is padded to one:
 *     acc | wsum | tile input | tile output | ramp table | ens [3][4H][4W]
 * ens holds the fp32 ensemble image when the call has run; acc and wsum the last variant's un-normalised canvas. */
long long ff_image_workspace_bytes(void* handle, int H, int W);
int ff_forward_image_u8(void* handle, const unsigned char* img_dev, int H, int W, int overlap, unsigned char* out_dev, void* work,
                        long long work_bytes, void* stream);
long long ff_image_ens_workspace_bytes(void* handle, int H, int W);
int ff_forward_image_ens_u8(void* handle, const unsigned char* img_dev, int H, int W, int overlap, const int* codes, int ncodes,
                            unsigned char* out_dev, void* work, long long work_bytes, void* stream);
int ff_create(const char* plan_path, void** out_handle);
int ff_upload(void* handle, const char* slot_name, const void* host_or_dev_ptr, long long nbytes);
int ff_finalize(void* handle);
int ff_forward(void* handle, const float* lr_dev, int B, int H, int W, float* out_dev, void* stream);
int ff_destroy(void* handle);
int ff_model_io_shape(void* handle, int* in_shape4, int* out_shape4);
int ff_model_num_slots(void* handle);
const char* ff_model_slot_name(void* handle, int i);
long long ff_model_slot_bytes(void* handle, int i);
long long ff_model_workspace_bytes(void* handle);
int ff_model_num_launches(void* handle);

#ifdef __cplusplus
}
#endif
#endif
