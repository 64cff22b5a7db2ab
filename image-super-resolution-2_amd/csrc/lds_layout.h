// Dynamic-LDS maps of the kernels whose image is not one of the named-macro maps (win_attn_layout.h, token_mlp_layout.h, and the
// XX_OFF_* blocks of hab_link.hip, ocab_attn.hip, chan_qkv.hip, sgfn_tail.hip, cab_fused.hip).  ONE definition per kernel: the kernel
// carves `smem + xx_off_*(...)`, its launcher passes `xx_lds(...)`, and tests/lds_layout_shim.cpp prints both on the host.  Byte
// offsets unless a name says floats.  Plain C++17: a function takes the template parameters or the run-time values (the kernel's p.
// fields, the launcher's arguments) the image depends on.
#pragma once
#include <stddef.h>

#ifndef FF_HD
#if defined(__HIPCC__)
#define FF_HD __host__ __device__ __forceinline__
#else
#define FF_HD inline
#endif
#endif

// nw wave-private patches of 32 rows x `row` floats: the row gather of ff_wave_rows_to_frags (FF_XS_ROW) and the 32 x 32 accumulator
// transposes of the epilogues (rows of 33, 34 or 36 floats)
#define FF_XS_ROW 68
FF_HD constexpr int ff_patches_bytes(int nw, int row) { return nw * 32 * row * 4; }

// ---- token_linear_kernel.inc: ring [2][hi | lo][32][2 ks + 1 slots] | tr [8][32][TL_TR] | xs [8][32][FF_XS_ROW] | vecs x [n_tiles * 32]
// floats: vector 0 the bias, vector 1 the column scale of the rows16 form.  tl_off_vec is the offset of vector i, tl_lds the launch size.
#define TL_TR 36   // floats per row of the transpose patch: 144 B keeps rows 16-byte aligned and ds_*_b128 conflict-free
FF_HD constexpr int tl_bufb(int ks) { return 2 * 32 * (2 * ks + 1) * 16; }
FF_HD constexpr int tl_off_tr(int ks) { return 2 * tl_bufb(ks); }
FF_HD constexpr int tl_off_xs(int ks) { return tl_off_tr(ks) + ff_patches_bytes(8, TL_TR); }
FF_HD constexpr size_t tl_off_vec(int ks, int n_tiles, int i) { return (size_t)(tl_off_xs(ks) + ff_patches_bytes(8, FF_XS_ROW)) + (size_t)i * n_tiles * 32 * 4; }
FF_HD constexpr size_t tl_lds(int ks, int n_tiles, int vecs) { return tl_off_vec(ks, n_tiles, vecs); }

// ---- naf_ffn_kernel (naf_fused.hip), c = 16 ks: W4 [4 planes][32][2 ks + 1 slots] | W5 [2 planes][c][80] | x_lo [8][32][32 ks + 16] |
// b4 [2 c] floats | x staging patches, present only where a wave's x_lo rows are too small to hold its patch (ks = 4)
FF_HD constexpr int nffn_w1b(int ks) { return 32 * (2 * ks + 1) * 16; }
FF_HD constexpr int nffn_w2b(int ks) { return 16 * ks * 5 * 16; }
FF_HD constexpr int nffn_xlrowb(int ks) { return ks * 32 + 16; }
FF_HD constexpr int nffn_off_w2(int ks) { return 4 * nffn_w1b(ks); }
FF_HD constexpr int nffn_off_xl(int ks) { return nffn_off_w2(ks) + 2 * nffn_w2b(ks); }
FF_HD constexpr int nffn_off_b4(int ks) { return nffn_off_xl(ks) + 8 * 32 * nffn_xlrowb(ks); }
FF_HD constexpr int nffn_off_xst(int ks) { return nffn_off_b4(ks) + 2 * 16 * ks * 4; }
FF_HD constexpr bool nffn_xs_in_xl(int ks) { return 32 * nffn_xlrowb(ks) >= ff_patches_bytes(1, FF_XS_ROW); }
FF_HD constexpr int nffn_lds(int ks) { return nffn_off_xst(ks) + (nffn_xs_in_xl(ks) ? 0 : ff_patches_bytes(8, FF_XS_ROW)); }

// ---- naf_front_kernel.inc, c channels: tile [NF_MT * 32][NF_TS] floats | W [2 tiles][32][4 c + 16] | red [8][8][4] floats |
// Wd [11][2 c] floats (nine depth-wise taps, depth-wise bias, conv1 bias)
#define NF_MT 6                           // m-tiles of 32 tokens (192 >= 180)
#define NF_TS 68                          // floats per token row of the LDS tile (64 + 4: conflict-free 16-byte rows)
FF_HD constexpr int nfr_wtileb(int c) { return 32 * (4 * c + 16); }
FF_HD constexpr int nfr_off_w() { return NF_MT * 32 * NF_TS * 4; }
FF_HD constexpr int nfr_off_red(int c) { return nfr_off_w() + 2 * nfr_wtileb(c); }
FF_HD constexpr int nfr_off_wd(int c) { return nfr_off_red(c) + 8 * 8 * 4 * 4; }
FF_HD constexpr int nfr_lds(int c) { return nfr_off_wd(c) + 11 * 2 * c * 4; }

// ---- naf_tail_kernel.inc, c = 16 ks, nw waves: W fragments [8 c c bytes] | constants [9 c] floats | patches [nw][32][cpp + 4] floats
// (cpp channels per gather pass: 64 at c = 64, else 32) | images form: one sca vector [c] per wave
FF_HD constexpr int ntl_xrow(int ks) { return (ks == 4 ? 64 : 32) + 4; }
FF_HD constexpr int ntl_off_cs(int ks) { return 8 * (16 * ks) * (16 * ks); }
FF_HD constexpr int ntl_off_xs(int ks) { return ntl_off_cs(ks) + 9 * 16 * ks * 4; }
FF_HD constexpr int ntl_off_sca(int ks, int nw) { return ntl_off_xs(ks) + ff_patches_bytes(nw, ntl_xrow(ks)); }
FF_HD constexpr int ntl_lds(int ks, int nw, bool img) { return ntl_off_sca(ks, nw) + (img ? nw * 16 * ks * 4 : 0); }

// ---- dwconv3_gate_pool_kernel (naf_pool_kernels.inc) and pool_partial_v4_kernel (norm_pool.hip): [rows][c / 4] float4 partial sums
FF_HD constexpr size_t pool4_lds(int rows, int cv) { return (size_t)rows * cv * 16; }
// ---- vec_mlp_kernel: xin [cin] | hid [ch];  pool_vec_mlp_kernel: red [16][cin rounded up to 64] | xin [cin] | hid [ch]  (floats)
FF_HD constexpr int vmlp_off_hid_f(int cin) { return cin; }
FF_HD constexpr size_t vmlp_lds(int cin, int ch) { return (size_t)(vmlp_off_hid_f(cin) + ch) * 4; }
FF_HD constexpr int pvm_cp(int cin) { return (cin + 63) & ~63; }
FF_HD constexpr int pvm_off_xin_f(int cin) { return 16 * pvm_cp(cin); }
FF_HD constexpr int pvm_off_hid_f(int cin) { return pvm_off_xin_f(cin) + cin; }
FF_HD constexpr size_t pvm_lds(int cin, int ch) { return (size_t)(pvm_off_hid_f(cin) + ch) * 4; }

// ---- window_attn_kernel (attention.hip), nkt key tiles of 32 (floats): K^T [32][32 nkt + 1] | V [32 nkt][32] | key regions [32 nkt]
FF_HD constexpr int wat_off_v_f(int nkt) { return 32 * (nkt * 32 + 1); }
FF_HD constexpr int wat_off_reg_f(int nkt) { return wat_off_v_f(nkt) + nkt * 32 * 32; }
FF_HD constexpr int wat_lds(int nkt) { return (wat_off_reg_f(nkt) + nkt * 32) * 4; }

// ---- window_attn_bf16_kernel (attention_bf16.hip): K hi | K lo [WAB_AKC][WAB_KROWB] | V^T hi | lo [32][WAB_VROWB] | key tokens [nkpad] | key
// regions [nkpad] | the head's relative-position table [rel_n] floats (rel_table only) | key offsets [nkpad] (rel_gen only).
// Epilogue: the waves' 32 x 34 transposes, then their query-token rows [8][32], over the idle K / V staging
#define WAB_AKC 128        // keys per chunk
#define WAB_KROWB 80       // K row: 32 bf16 + 16 B pad
#define WAB_VROWB 272      // V^T row: 128 bf16 + 16 B pad
#define WAB_OFF_KL (WAB_AKC * WAB_KROWB)
#define WAB_OFF_VH (2 * WAB_AKC * WAB_KROWB)
#define WAB_OFF_VL (WAB_OFF_VH + 32 * WAB_VROWB)
#define WAB_OFF_KTOK (WAB_OFF_VL + 32 * WAB_VROWB)
#define WAB_OFF_TOKQ (8 * 32 * 34 * 4)
static_assert(WAB_OFF_TOKQ + 8 * 32 * 4 <= WAB_OFF_KTOK, "attention_bf16: epilogue patches and query rows must fit in the K / V staging");
FF_HD constexpr size_t wab_off_kreg(int nkpad) { return (size_t)WAB_OFF_KTOK + (size_t)nkpad * 4; }
FF_HD constexpr size_t wab_off_rel(int nkpad) { return wab_off_kreg(nkpad) + (size_t)nkpad * 4; }
FF_HD constexpr size_t wab_off_kofs(int nkpad, int rel_n, bool rel) { return wab_off_rel(nkpad) + (rel ? (size_t)rel_n * 4 : 0); }
FF_HD constexpr size_t wab_lds(int nkpad, int rel_n, bool rel, bool rel_gen) { return wab_off_kofs(nkpad, rel_n, rel) + (rel_gen ? (size_t)nkpad * 4 : 0); }

// ---- the tiled GEMMs: [2 buffers][A tile bm rows | B tile bn rows] of rowb bytes per row.  conv_igemm_kernel (conv_gemm.hip): 80 B
// (CG_LDK floats); conv_igemm_bf16_kernel.inc: [bkb hi | bkb lo | 16 B pad]; gemm_rows_bf16.hip: 128 B.  The bf16 kernels' epilogues lay
// wm * wn 32 x 36 transpose patches over the idle ring.
#define CG_LDK 20
FF_HD constexpr int cig_rowb(int bkb) { return bkb * 4 + 16; }
#define RG_ROWB 128
FF_HD constexpr int gemm_off_b(int bm, int rowb) { return 2 * bm * rowb; }           // layout [2][bm] then [2][bn] (the conv kernels)
FF_HD constexpr int gemm_bufb(int bm, int bn, int rowb) { return (bm + bn) * rowb; }   // one buffer of the [2][A tile | B tile] form (gemm_rows_bf16.hip)
FF_HD constexpr int gemm_lds(int bm, int bn, int rowb) { return 2 * gemm_bufb(bm, bn, rowb); }
FF_HD constexpr bool gemm_patches_fit(int bm, int bn, int rowb, int nw) { return ff_patches_bytes(nw, 36) <= gemm_lds(bm, bn, rowb); }

// ---- conv3x3_halo_kernel: X [th + 2 rows][prow] | W ring [nslot][wslot], wslot = bn weight rows of wrow bytes rounded up to 1-KiB DMA
// pieces.  Epilogues over the idle staging: the pool row [wm][bn] floats at 0; the vector epilogue's patches at HALO_OFF_PATCH
FF_HD constexpr int halo_wrow(int wk, int nterms) { return (nterms == 1 ? wk * 2 : wk * 4) + 16; }
FF_HD constexpr int halo_wslot(int bn, int wk, int nterms) { return (bn * halo_wrow(wk, nterms) + 1023) / 1024 * 1024; }
FF_HD constexpr int halo_off_w(int th, int prow) { return (th + 2) * prow; }
FF_HD constexpr int halo_lds(int th, int prow, int nslot, int wslot) { return halo_off_w(th, prow) + nslot * wslot; }
#define HALO_OFF_PATCH 8192
FF_HD constexpr bool halo_epilogue_fits(int wm, int wn, int bn, int lds) {
  return wm * bn * 4 <= HALO_OFF_PATCH && HALO_OFF_PATCH + ff_patches_bytes(wm * wn, 36) <= lds;
}

// ---- conv3x3_small_kernel: the 18 x 18 halo tile, cinp + 4 floats per pixel
FF_HD constexpr size_t c3s_lds(int cinp) { return (size_t)324 * (cinp + 4) * 4; }

// ---- freq.hip (floats): rdft_rows_kernel row [w] | cos [w] | sin [w];  cdft_cols_kernel tile [h][cb][2] | cos [h] | sin [h];
// the inverse row kernels (freq_irdft_row.inc) urow [wf][2] | cos [w] | sin [w]
FF_HD constexpr int rdft_off_cos_f(int w) { return w; }
FF_HD constexpr int rdft_off_sin_f(int w) { return 2 * w; }
FF_HD constexpr size_t rdft_lds(int w) { return (size_t)w * 12; }
FF_HD constexpr int cdft_off_cos_f(int h, int cb) { return 2 * h * cb; }
FF_HD constexpr int cdft_off_sin_f(int h, int cb) { return cdft_off_cos_f(h, cb) + h; }
FF_HD constexpr size_t cdft_lds(int h, int cb) { return (size_t)h * cb * 8 + (size_t)h * 8; }
FF_HD constexpr int irdft_off_cos_f(int wf) { return 2 * wf; }
FF_HD constexpr int irdft_off_sin_f(int wf, int w) { return irdft_off_cos_f(wf) + w; }
FF_HD constexpr size_t irdft_lds(int wf, int w) { return (size_t)wf * 8 + (size_t)w * 8; }
