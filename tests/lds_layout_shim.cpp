// Host build of the kernels' LDS maps (csrc/lds_layout.h, token_mlp_layout.h, win_attn_layout.h): prints "expression value" per line
// for the cases tests/test_lds_layout_cpu.py pins to literal byte counts.  No HIP.
#include <stdio.h>

#include "lds_layout.h"
#include "token_mlp_layout.h"
#include "win_attn_layout.h"

#define P(e) printf("%s %lld\n", #e, (long long)(e))

// one instantiation of conv3x3_halo.hip's launch_halo<WM, WN, MI, NI, WK, NSLOT, NTERMS>: its launch size, and whether its two epilogues'
// patches fit in it.  The tile-row pitch is HaloGeom<NTERMS>::PROW of that file: 2816 bytes for plain bf16, HX_PROW = 5120 for split
static void halo(int wm, int wn, int mi, int ni, int wk, int nslot, int nterms) {
  const int th = wm * mi * 2, bn = wn * ni * 32, prow = nterms == 1 ? 2816 : 5120;
  const int lds = halo_lds(th, prow, nslot, halo_wslot(bn, wk, nterms));
  printf("halo<%d,%d,%d,%d,%d,%d,%d>.lds %d\n", wm, wn, mi, ni, wk, nslot, nterms, lds);
  printf("halo<%d,%d,%d,%d,%d,%d,%d>.vec_epilogue_fits %d\n", wm, wn, mi, ni, wk, nslot, nterms, (int)halo_epilogue_fits(wm, wn, bn, lds));
  printf("halo<%d,%d,%d,%d,%d,%d,%d>.pool_row_fits %d\n", wm, wn, mi, ni, wk, nslot, nterms, (int)(wm * bn * 4 <= halo_off_w(th, prow)));
}

int main() {
  // ---- token_linear: (ks, n_tiles, vectors)
  P(tl_bufb(12)); P(tl_off_tr(12)); P(tl_off_xs(12)); P(tl_off_vec(12, 17, 0)); P(tl_off_vec(12, 17, 1));
  P(tl_off_vec(12, 1, 1)); P(tl_off_vec(12, 6, 1)); P(tl_off_vec(12, 12, 1)); P(tl_off_vec(12, 23, 1)); P(tl_off_vec(12, 48, 1)); P(tl_off_vec(12, 49, 1));
  P(tl_off_vec(4, 4, 1)); P(tl_off_vec(4, 1, 1)); P(tl_off_vec(4, 304, 1)); P(tl_off_vec(4, 305, 1));
  P(tl_off_vec(8, 8, 1)); P(tl_off_vec(8, 1, 1)); P(tl_off_vec(8, 176, 1)); P(tl_off_vec(8, 177, 1));
  P(tl_off_vec(12, 17, 2)); P(tl_off_vec(12, 1, 2)); P(tl_off_vec(12, 24, 2)); P(tl_off_vec(12, 25, 2));
  P(tl_lds(12, 17, 1)); P(tl_lds(12, 17, 2)); P(tl_lds(4, 4, 2)); P(tl_lds(4, 1, 2)); P(tl_lds(4, 152, 2)); P(tl_lds(4, 153, 2));
  P(tl_lds(8, 8, 2)); P(tl_lds(8, 1, 2)); P(tl_lds(8, 88, 2)); P(tl_lds(8, 89, 2));
  // ---- token_mlp / token_projmlp (split), token_projmlp_bf16
  P(TM_OFF_W2); P(TM_OFF_XL); P(TM_OFF_B1); P(TM_LDS(1)); P(TM_LDS(12)); P(TM_LDS(40)); P(TM_LDS(41));
  P(PM_OFF_VEC); P(PM_OFF_BT); P(PM_OFF_SC); P(PM_OFF_BP); P(PM_OFF_B1); P(PM_LDS(1)); P(PM_LDS(12)); P(PM_LDS(88)); P(PM_LDS(89));
  P(TM_TRB(36)); P(TM_TRB(33)); P(32 * FF_XS_ROW * 4); P(32 * XLROWB); P(W1PIECES * 1024); P(2 * TM_W1B); P(2 * TM_W2B);
  P(PM_OFF_W2 + 2 * PM_W2SLOT); P(PM_PROJB);
  // ---- NAFNet
  P(nffn_off_w2(4)); P(nffn_off_xl(4)); P(nffn_off_b4(4)); P(nffn_off_xst(4)); P(nffn_xs_in_xl(4)); P(nffn_lds(4));
  P(nffn_off_w2(8)); P(nffn_off_xl(8)); P(nffn_off_b4(8)); P(nffn_off_xst(8)); P(nffn_xs_in_xl(8)); P(nffn_lds(8));
  P(ff_patches_bytes(8, 33)); P(ff_patches_bytes(1, FF_XS_ROW)); P(32 * nffn_xlrowb(4)); P(32 * nffn_xlrowb(8));
  P(nfr_off_w()); P(nfr_off_red(64)); P(nfr_off_wd(64)); P(nfr_lds(64)); P(nfr_off_red(128)); P(nfr_off_wd(128)); P(nfr_lds(128));
  P(ntl_off_cs(4)); P(ntl_off_xs(4)); P(ntl_off_sca(4, 4)); P(ntl_lds(4, 4, false)); P(ntl_lds(4, 4, true)); P(ntl_xrow(4));
  P(ntl_off_cs(8)); P(ntl_off_xs(8)); P(ntl_off_sca(8, 4)); P(ntl_lds(8, 4, false)); P(ntl_lds(8, 4, true)); P(ntl_xrow(8));
  P(pool4_lds(16, 16)); P(pool4_lds(8, 32)); P(pool4_lds(1, 256)); P(pool4_lds(64, 1));
  P(vmlp_off_hid_f(180)); P(vmlp_lds(180, 6)); P(pvm_cp(180)); P(pvm_off_xin_f(180)); P(pvm_off_hid_f(180)); P(pvm_lds(180, 6)); P(pvm_lds(64, 64)); P(pvm_lds(1, 1));
  // ---- attention
  P(wat_off_v_f(4)); P(wat_off_reg_f(4)); P(wat_lds(4));
  P(WAB_OFF_KL); P(WAB_OFF_VH); P(WAB_OFF_VL); P(WAB_OFF_KTOK); P(WAB_OFF_TOKQ); P(WAB_OFF_TOKQ + 8 * 32 * 4);
  P(wab_off_kreg(256)); P(wab_off_rel(256)); P(wab_off_kofs(256, 961, true)); P(wab_off_kofs(256, 961, false));
  P(wab_lds(256, 961, false, false)); P(wab_lds(256, 961, true, false)); P(wab_lds(640, 1521, true, true)); P(wab_lds(640, 1521, false, false));
  P(wab_lds(128, 0, false, false)); P(wab_lds(3456, 0, false, false)); P(wab_lds(3584, 0, false, false));
  P(WF_LDS); P(W2_LDS);
  // ---- tiled GEMMs
  P(gemm_off_b(128, CG_LDK)); P(gemm_lds(128, 128, CG_LDK * 4)); P(gemm_lds(256, 32, CG_LDK * 4)); P(gemm_lds(128, 64, CG_LDK * 4));
  P(cig_rowb(32)); P(cig_rowb(64)); P(gemm_off_b(256, cig_rowb(32))); P(gemm_lds(256, 192, cig_rowb(32))); P(gemm_lds(128, 128, cig_rowb(64)));
  P(gemm_lds(256, 32, cig_rowb(32))); P(gemm_lds(128, 64, cig_rowb(32))); P(gemm_lds(128, 64, cig_rowb(64)));
  P(gemm_lds(128, 128, cig_rowb(32))); P(gemm_lds(256, 128, cig_rowb(32)));
  P(gemm_bufb(128, 128, RG_ROWB)); P(gemm_lds(128, 128, RG_ROWB)); P(gemm_lds(128, 64, RG_ROWB));
  // the epilogue patches of every launched (BM, BN, row, WM * WN): conv_gemm_bf16.hip cfg 1 .. 9, gemm_rows_bf16.hip cfg 1, 2
  P(gemm_patches_fit(128, 128, cig_rowb(32), 4)); P(gemm_patches_fit(128, 64, cig_rowb(32), 4)); P(gemm_patches_fit(256, 32, cig_rowb(32), 4));
  P(gemm_patches_fit(256, 192, cig_rowb(32), 8)); P(gemm_patches_fit(128, 128, cig_rowb(32), 8)); P(gemm_patches_fit(256, 128, cig_rowb(32), 8));
  P(gemm_patches_fit(128, 128, cig_rowb(64), 8)); P(gemm_patches_fit(128, 64, cig_rowb(64), 8));
  P(gemm_patches_fit(128, 128, RG_ROWB, 8)); P(gemm_patches_fit(128, 64, RG_ROWB, 8));
  P(ff_patches_bytes(8, 36)); P(ff_patches_bytes(4, 36)); P(gemm_patches_fit(128, 64, cig_rowb(32), 8)); P(gemm_patches_fit(64, 32, RG_ROWB, 8));
  // ---- 3x3 convolutions
  P(halo_wrow(64, 1)); P(halo_wrow(64, 3)); P(halo_wrow(32, 1)); P(halo_wrow(32, 3));
  P(halo_wslot(32, 64, 1)); P(halo_wslot(64, 64, 1)); P(halo_wslot(128, 64, 1)); P(halo_wslot(192, 32, 1));
  P(halo_wslot(32, 64, 3)); P(halo_wslot(64, 64, 3)); P(halo_wslot(128, 64, 3)); P(halo_wslot(192, 32, 3));
  P(halo_off_w(8, 2816)); P(halo_off_w(16, 2816)); P(halo_off_w(8, 5120)); P(halo_off_w(16, 5120));
  halo(8, 1, 1, 2, 64, 9, 1); halo(4, 1, 1, 1, 64, 2, 1);                                 // the small-grid forms
  halo(8, 1, 1, 1, 64, 2, 3); halo(8, 1, 1, 1, 64, 2, 1); halo(8, 1, 1, 2, 64, 2, 3); halo(8, 1, 1, 2, 64, 2, 1);
  halo(2, 2, 2, 2, 64, 2, 3); halo(2, 2, 2, 2, 64, 2, 1); halo(4, 2, 2, 3, 32, 2, 3); halo(4, 2, 2, 3, 32, 2, 1);
  P(HALO_OFF_PATCH); P(halo_epilogue_fits(4, 1, 32, 38400)); P(halo_epilogue_fits(4, 1, 32, 8192 + 18431)); P(halo_epilogue_fits(8, 1, 288, 163840));
  P(c3s_lds(4)); P(c3s_lds(64)); P(c3s_lds(124)); P(c3s_lds(128));
  // ---- frequency kernels
  P(rdft_off_cos_f(256)); P(rdft_off_sin_f(256)); P(rdft_lds(256)); P(rdft_lds(2)); P(rdft_lds(5461)); P(rdft_lds(5462)); P(rdft_lds(8192)); P(cdft_off_sin_f(256, 16)); P(cdft_off_cos_f(256, 16)); P(cdft_lds(256, 16)); P(cdft_lds(481, 16)); P(cdft_lds(482, 16)); P(cdft_lds(513, 4)); P(cdft_lds(1638, 4)); P(cdft_lds(1639, 4));
  P(irdft_off_cos_f(129)); P(irdft_off_sin_f(129, 256)); P(irdft_lds(129, 256)); P(irdft_lds(2, 2)); P(irdft_lds(2731, 5461)); P(irdft_lds(2732, 5462)); P(irdft_lds(4097, 8192));
  return 0;
}
