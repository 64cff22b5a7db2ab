"""The kernels' LDS maps (csrc/lds_layout.h, token_mlp_layout.h), on the host: tests/lds_layout_shim.cpp is built with the host compiler
and prints offsets and launch byte counts for the shapes the product launches and for the edges of every run-time parameter.  The
expected values are LITERALS worked out from the launcher formulas of the commit before the maps existed (each formula stands beside
its value, with the file and line it was read from), so a map that drifts from what was launched fails here.  No HIP, no GPU.

Every patch an epilogue or prologue lays over another area is checked to end inside that area.  The over-limit side goes through the
real entry points, as refusals only: host addresses, FF_ERR_ARG and the pinned message -- no call here passes every check."""
import ctypes
import os
import subprocess

import pytest

from test_device_once_cpu import ROOT, _host_compiler

LDS_MAX = 163840          # 160 KiB: FF_LDS_MAX
LDS_DEFAULT_MAX = 65536   # what a launch gets without raising the attribute: FF_LDS_DEFAULT_MAX

EXPECTED = {
    # token_linear.hip:88 parent: 2*2*32*(2*ks+1)*16 + 8*32*TL_TR*4 + 8*32*FF_XS_ROW*4 + n_tiles*32*4 (rows16 :136: 2*n_tiles; gated :172: the literal 25)
    'tl_bufb(12)': 25600,                                  # 2*32*25*16
    'tl_off_tr(12)': 51200,                                # 2*2*32*25*16
    'tl_off_xs(12)': 88064,                                # 2*2*32*25*16 + 8*32*36*4
    'tl_off_vec(12, 17, 0)': 157696,                       # 2*2*32*25*16 + 8*32*36*4 + 8*32*68*4
    'tl_off_vec(12, 17, 1)': 159872,                       # 51200 + 36864 + 69632 + 17*32*4
    'tl_off_vec(12, 1, 1)': 157824,                        # 51200 + 36864 + 69632 + 1*32*4
    'tl_off_vec(12, 6, 1)': 158464,                        # 51200 + 36864 + 69632 + 6*32*4
    'tl_off_vec(12, 12, 1)': 159232,                       # 51200 + 36864 + 69632 + 12*32*4
    'tl_off_vec(12, 23, 1)': 160640,                       # 51200 + 36864 + 69632 + 23*32*4
    'tl_off_vec(12, 48, 1)': 163840,                       # 51200 + 36864 + 69632 + 48*32*4
    'tl_off_vec(12, 49, 1)': 163968,                       # 51200 + 36864 + 69632 + 49*32*4
    'tl_off_vec(4, 4, 1)': 125440,                         # 2*2*32*9*16 + 36864 + 69632 + 4*32*4
    'tl_off_vec(4, 1, 1)': 125056,                         # 2*2*32*9*16 + 36864 + 69632 + 1*32*4
    'tl_off_vec(4, 304, 1)': 163840,                       # 2*2*32*9*16 + 36864 + 69632 + 304*32*4
    'tl_off_vec(4, 305, 1)': 163968,                       # 2*2*32*9*16 + 36864 + 69632 + 305*32*4
    'tl_off_vec(8, 8, 1)': 142336,                         # 2*2*32*17*16 + 36864 + 69632 + 8*32*4
    'tl_off_vec(8, 1, 1)': 141440,                         # 2*2*32*17*16 + 36864 + 69632 + 1*32*4
    'tl_off_vec(8, 176, 1)': 163840,                       # 2*2*32*17*16 + 36864 + 69632 + 176*32*4
    'tl_off_vec(8, 177, 1)': 163968,                       # 2*2*32*17*16 + 36864 + 69632 + 177*32*4
    'tl_off_vec(12, 17, 2)': 162048,                       # 51200 + 36864 + 69632 + 2*17*32*4
    'tl_off_vec(12, 1, 2)': 157952,                        # 51200 + 36864 + 69632 + 2*1*32*4
    'tl_off_vec(12, 24, 2)': 163840,                       # 51200 + 36864 + 69632 + 2*24*32*4
    'tl_off_vec(12, 25, 2)': 164096,                       # 51200 + 36864 + 69632 + 2*25*32*4
    'tl_lds(12, 17, 1)': 159872,                           # 51200 + 36864 + 69632 + 17*32*4
    'tl_lds(12, 17, 2)': 162048,                           # 51200 + 36864 + 69632 + 2*17*32*4
    'tl_lds(4, 4, 2)': 125952,                             # 2*2*32*9*16 + 36864 + 69632 + 2*4*32*4
    'tl_lds(4, 1, 2)': 125184,                             # 2*2*32*9*16 + 36864 + 69632 + 2*1*32*4
    'tl_lds(4, 152, 2)': 163840,                           # 2*2*32*9*16 + 36864 + 69632 + 2*152*32*4
    'tl_lds(4, 153, 2)': 164096,                           # 2*2*32*9*16 + 36864 + 69632 + 2*153*32*4
    'tl_lds(8, 8, 2)': 143360,                             # 2*2*32*17*16 + 36864 + 69632 + 2*8*32*4
    'tl_lds(8, 1, 2)': 141568,                             # 2*2*32*17*16 + 36864 + 69632 + 2*1*32*4
    'tl_lds(8, 88, 2)': 163840,                            # 2*2*32*17*16 + 36864 + 69632 + 2*88*32*4
    'tl_lds(8, 89, 2)': 164096,                            # 2*2*32*17*16 + 36864 + 69632 + 2*89*32*4
    # token_mlp.hip:574 / :628 parent: (2*W1PL + 2*W2PL)*16 + 8*32*XLROWB + hidden_tiles*32*4, W1PL 800, W2PL 960, XLROWB 400
    'TM_OFF_W2': 25600,                                    # 2*800*16
    'TM_OFF_XL': 56320,                                    # (2*800 + 2*960)*16
    'TM_OFF_B1': 158720,                                   # (2*800 + 2*960)*16 + 8*32*400
    'TM_LDS(1)': 158848,                                   # 56320 + 102400 + 1*32*4
    'TM_LDS(12)': 160256,                                  # 56320 + 102400 + 12*32*4
    'TM_LDS(40)': 163840,                                  # 56320 + 102400 + 40*32*4
    'TM_LDS(41)': 163968,                                  # 56320 + 102400 + 41*32*4
    # token_mlp.hip:583 parent: PM_OFF_VEC + (4*TM_KP + hidden_tiles*32)*4, PM_OFF_VEC = 6*13*1024 + 8*32*68*4
    'PM_OFF_VEC': 149504,                                  # 6*13*1024 + 8*32*68*4
    'PM_OFF_BT': 150272,                                   # 149504 + 192*4
    'PM_OFF_SC': 151040,                                   # 149504 + 2*192*4
    'PM_OFF_BP': 151808,                                   # 149504 + 3*192*4
    'PM_OFF_B1': 152576,                                   # 149504 + 4*192*4
    'PM_LDS(1)': 152704,                                   # 149504 + (4*192 + 1*32)*4
    'PM_LDS(12)': 154112,                                  # 149504 + (4*192 + 12*32)*4
    'PM_LDS(88)': 163840,                                  # 149504 + (4*192 + 88*32)*4
    'PM_LDS(89)': 163968,                                  # 149504 + (4*192 + 89*32)*4
    # NAFNet.  naf_fused.hip:281 parent: 4*32*(2*KS+1)*16 + 2*C*5*16 + 8*32*(KS*32+16) + 2*C*4 + (KS >= 8 ? 0 : 8*32*FF_XS_ROW*4)
    'nffn_off_w2(4)': 18432,                               # 4*32*9*16
    'nffn_off_xl(4)': 28672,                               # 4*32*9*16 + 2*64*5*16
    'nffn_off_b4(4)': 65536,                               # 4*32*9*16 + 2*64*5*16 + 8*32*144
    'nffn_off_xst(4)': 66048,                              # 4*32*9*16 + 2*64*5*16 + 8*32*144 + 2*64*4
    'nffn_xs_in_xl(4)': 0,                                 # 0
    'nffn_lds(4)': 135680,                                 # 4*32*9*16 + 2*64*5*16 + 8*32*144 + 2*64*4 + 8*32*68*4
    'nffn_off_w2(8)': 34816,                               # 4*32*17*16
    'nffn_off_xl(8)': 55296,                               # 4*32*17*16 + 2*128*5*16
    'nffn_off_b4(8)': 124928,                              # 4*32*17*16 + 2*128*5*16 + 8*32*272
    'nffn_off_xst(8)': 125952,                             # 4*32*17*16 + 2*128*5*16 + 8*32*272 + 2*128*4
    'nffn_xs_in_xl(8)': 1,                                 # 1
    'nffn_lds(8)': 125952,                                 # 4*32*17*16 + 2*128*5*16 + 8*32*272 + 2*128*4 + 0
    # naf_front.inc:75 parent: NF_MT*32*NF_TS*4 + 2*32*(4*C+16) + 8*8*4*4 + 11*2*C*4
    'nfr_off_w()': 52224,                                  # 6*32*68*4
    'nfr_off_red(64)': 69632,                              # 6*32*68*4 + 2*32*(4*64+16)
    'nfr_off_wd(64)': 70656,                               # 6*32*68*4 + 2*32*(4*64+16) + 8*8*4*4
    'nfr_lds(64)': 76288,                                  # 6*32*68*4 + 2*32*(4*64+16) + 8*8*4*4 + 11*2*64*4
    'nfr_off_red(128)': 86016,                             # 6*32*68*4 + 2*32*(4*128+16)
    'nfr_off_wd(128)': 87040,                              # 6*32*68*4 + 2*32*(4*128+16) + 8*8*4*4
    'nfr_lds(128)': 98304,                                 # 6*32*68*4 + 2*32*(4*128+16) + 8*8*4*4 + 11*2*128*4
    # naf_tail.hip:69 parent: 8*C*C + 9*C*4 + NW*32*((KS == 4 ? 64 : 32) + 4)*4 + (IMG ? NW*C*4 : 0); its table: 69 888, 70 912, 154 112, 156 160
    'ntl_off_cs(4)': 32768,                                # 8*64*64
    'ntl_off_xs(4)': 35072,                                # 8*64*64 + 9*64*4
    'ntl_off_sca(4, 4)': 69888,                            # 8*64*64 + 9*64*4 + 4*32*68*4
    'ntl_lds(4, 4, false)': 69888,                         # 69888
    'ntl_lds(4, 4, true)': 70912,                          # 70912
    'ntl_xrow(4)': 68,                                     # 64 + 4
    'ntl_off_cs(8)': 131072,                               # 8*128*128
    'ntl_off_xs(8)': 135680,                               # 8*128*128 + 9*128*4
    'ntl_off_sca(8, 4)': 154112,                           # 8*128*128 + 9*128*4 + 4*32*36*4
    'ntl_lds(8, 4, false)': 154112,                        # 154112
    'ntl_lds(8, 4, true)': 156160,                         # 156160
    'ntl_xrow(8)': 36,                                     # 32 + 4
    # naf_fused.hip:50 and norm_pool.hip:178 parent: rows*cv*16;  norm_pool.hip:299 (Cin+Ch)*4;  :377 (16*((Cin+63)&~63) + Cin + Ch)*4
    'pool4_lds(16, 16)': 4096,                             # 16*16*16
    'pool4_lds(8, 32)': 4096,                              # 8*32*16
    'pool4_lds(1, 256)': 4096,                             # 1*256*16
    'pool4_lds(64, 1)': 1024,                              # 64*1*16
    'vmlp_off_hid_f(180)': 180,                            # 180
    'vmlp_lds(180, 6)': 744,                               # (180+6)*4
    'pvm_off_hid_f(180)': 3252,                            # 16*192 + 180
    'pvm_cp(180)': 192,                                    # 192
    'pvm_off_xin_f(180)': 3072,                            # 16*192
    'pvm_lds(180, 6)': 13032,                              # (16*192 + 180 + 6)*4
    'pvm_lds(64, 64)': 4608,                               # (16*64 + 64 + 64)*4
    'pvm_lds(1, 1)': 4104,                                 # (16*64 + 1 + 1)*4
    # attention.hip:205 parent: (32*(NKT*32+1) + NKT*32*32)*4 + NKT*32*4
    'wat_off_v_f(4)': 4128,                                # 32*129
    'wat_off_reg_f(4)': 8224,                              # 32*129 + 128*32
    'wat_lds(4)': 33408,                                   # (32*129 + 128*32)*4 + 128*4
    # attention_bf16.hip:354 parent: 2*AKC*KROWB + 2*32*VROWB + 2*nkpad*4 + (rel_table ? rel_n*4 : 0) + (rel_gen ? nkpad*4 : 0); 128, 80, 272
    'WAB_OFF_KL': 10240,                                   # 128*80
    'WAB_OFF_VH': 20480,                                   # 2*128*80
    'WAB_OFF_VL': 29184,                                   # 2*128*80 + 32*272
    'WAB_OFF_KTOK': 37888,                                 # 2*128*80 + 2*32*272
    'WAB_OFF_TOKQ': 34816,                                 # 8*32*34*4
    'wab_off_kreg(256)': 38912,                            # 37888 + 256*4
    'wab_off_rel(256)': 39936,                             # 37888 + 2*256*4
    'wab_off_kofs(256, 961, true)': 43780,                 # 37888 + 2*256*4 + 961*4
    'wab_off_kofs(256, 961, false)': 39936,                # 37888 + 2*256*4
    'wab_lds(256, 961, false, false)': 39936,              # 37888 + 2*256*4
    'wab_lds(256, 961, true, false)': 43780,               # 37888 + 2*256*4 + 961*4
    'wab_lds(640, 1521, true, true)': 51652,               # 37888 + 2*640*4 + 1521*4 + 640*4
    'wab_lds(640, 1521, false, false)': 43008,             # 37888 + 2*640*4
    'wab_lds(128, 0, false, false)': 38912,                # 37888 + 2*128*4
    'wab_lds(3456, 0, false, false)': 65536,               # 37888 + 2*3456*4
    'wab_lds(3584, 0, false, false)': 66560,               # 37888 + 2*3584*4
    # win_attn_layout.h, unchanged: WF_LDS and W2_LDS as the parent's macros give them
    'WF_LDS': 140848,                                      # 2*25600 + 8*5120 + 2*32*528 + 2564*4 + 576*4 + 1024 + 1024 + 288
    'W2_LDS': 138816,                                      # 38*1024 + 2*8*2560 + 2*32*528 + 2*2564*4 + 576*4 + 1024 + 1024 + 288
    # conv_gemm.hip:196 parent: 2*(BM+BN)*LDK*4, LDK 20;  conv_gemm_bf16.hip:74 / :102: 2*(BM+BN)*(BKB*4+16);  gemm_rows_bf16.hip:245: 2*(BM+BN)*128
    'gemm_off_b(128, CG_LDK)': 5120,                       # 2*128*20
    'gemm_lds(128, 128, CG_LDK * 4)': 40960,               # 2*(128+128)*20*4
    'gemm_lds(256, 32, CG_LDK * 4)': 46080,                # 2*(256+32)*20*4
    'gemm_lds(128, 64, CG_LDK * 4)': 30720,                # 2*(128+64)*20*4
    'cig_rowb(32)': 144,                                   # 32*4 + 16
    'cig_rowb(64)': 272,                                   # 64*4 + 16
    'gemm_off_b(256, cig_rowb(32))': 73728,                # 2*256*144
    'gemm_lds(256, 192, cig_rowb(32))': 129024,            # 2*(256+192)*144
    'gemm_lds(128, 128, cig_rowb(64))': 139264,            # 2*(128+128)*272
    'gemm_lds(256, 32, cig_rowb(32))': 82944,              # 2*(256+32)*144
    'gemm_lds(128, 64, cig_rowb(32))': 55296,              # 2*(128+64)*144
    'gemm_lds(128, 64, cig_rowb(64))': 104448,             # 2*(128+64)*272
    'gemm_lds(128, 128, cig_rowb(32))': 73728,             # 2*(128+128)*144
    'gemm_bufb(128, 128, RG_ROWB)': 32768,                 # (128+128)*128
    'gemm_lds(128, 128, RG_ROWB)': 65536,                  # 2*(128+128)*128
    'gemm_lds(256, 128, cig_rowb(32))': 110592,            # 2*(256+128)*144
    'gemm_lds(128, 64, RG_ROWB)': 49152,                   # 2*(128+64)*128
    # conv3x3_halo.hip:380-381 parent: WSLOT = ((BN*((NTERMS == 1 ? WK*2 : WK*4) + 16) + 1023)/1024)*1024; lds = (TH+2)*PROW + NSLOT*WSLOT, TH = 2*WM*MI, BN = 32*WN*NI, PROW 2816 (NTERMS 1) or 5120
    'halo_wrow(64, 1)': 144,                               # 64*2 + 16
    'halo_wrow(64, 3)': 272,                               # 64*4 + 16
    'halo_wrow(32, 1)': 80,                                # 32*2 + 16
    'halo_wrow(32, 3)': 144,                               # 32*4 + 16
    'halo_wslot(32, 64, 1)': 5120,                         # ((32*144 + 1023)//1024)*1024
    'halo_wslot(64, 64, 1)': 9216,                         # ((64*144 + 1023)//1024)*1024
    'halo_wslot(128, 64, 1)': 18432,                       # ((128*144 + 1023)//1024)*1024
    'halo_wslot(192, 32, 1)': 15360,                       # ((192*80 + 1023)//1024)*1024
    'halo_wslot(32, 64, 3)': 9216,                         # ((32*272 + 1023)//1024)*1024
    'halo_wslot(64, 64, 3)': 17408,                        # ((64*272 + 1023)//1024)*1024
    'halo_wslot(128, 64, 3)': 34816,                       # ((128*272 + 1023)//1024)*1024
    'halo_wslot(192, 32, 3)': 27648,                       # ((192*144 + 1023)//1024)*1024
    'halo_off_w(8, 2816)': 28160,                          # 10*2816
    'halo_off_w(16, 2816)': 50688,                         # 18*2816
    'halo_off_w(8, 5120)': 51200,                          # 10*5120
    'halo_off_w(16, 5120)': 92160,                         # 18*5120
    # one total per instantiation of launch_halo<WM, WN, MI, NI, WK, NSLOT, NTERMS> (conv3x3_halo.hip:457-466)
    'halo<8,1,1,2,64,9,1>.lds': 133632,                    # 18*2816 + 9*9216
    'halo<4,1,1,1,64,2,1>.lds': 38400,                     # 10*2816 + 2*5120
    'halo<8,1,1,1,64,2,3>.lds': 110592,                    # 18*5120 + 2*9216
    'halo<8,1,1,1,64,2,1>.lds': 60928,                     # 18*2816 + 2*5120
    'halo<8,1,1,2,64,2,3>.lds': 126976,                    # 18*5120 + 2*17408
    'halo<8,1,1,2,64,2,1>.lds': 69120,                     # 18*2816 + 2*9216
    'halo<2,2,2,2,64,2,3>.lds': 120832,                    # 10*5120 + 2*34816
    'halo<2,2,2,2,64,2,1>.lds': 65024,                     # 10*2816 + 2*18432
    'halo<4,2,2,3,32,2,3>.lds': 147456,                    # 18*5120 + 2*27648
    'halo<4,2,2,3,32,2,1>.lds': 81408,                     # 18*2816 + 2*15360
    'HALO_OFF_PATCH': 8192,                                # 8192
    # conv3x3_small.hip:81 parent: 324*(CinP+4)*4
    'c3s_lds(4)': 10368,                                   # 324*8*4
    'c3s_lds(64)': 88128,                                  # 324*68*4
    'c3s_lds(124)': 165888,                                # 324*128*4
    'c3s_lds(128)': 171072,                                # 324*132*4
    # freq.hip parent: :283 W*12;  :278 / :347 H*CB*8 + H*8 (64 KiB limit);  :294 / :379 Wf*8 + W*8
    'rdft_off_cos_f(256)': 256,                            # 256
    'rdft_off_sin_f(256)': 512,                            # 2*256
    'rdft_lds(256)': 3072,                                 # 256*12
    'rdft_lds(2)': 24,                                     # 2*12
    'rdft_lds(5461)': 65532,                               # 5461*12
    'rdft_lds(5462)': 65544,                               # 5462*12
    'rdft_lds(8192)': 98304,                               # 8192*12
    'cdft_off_sin_f(256, 16)': 8448,                       # 2*256*16 + 256
    'cdft_off_cos_f(256, 16)': 8192,                       # 2*256*16
    'cdft_lds(256, 16)': 34816,                            # 256*16*8 + 256*8
    'cdft_lds(481, 16)': 65416,                            # 481*16*8 + 481*8
    'cdft_lds(482, 16)': 65552,                            # 482*16*8 + 482*8
    'cdft_lds(513, 4)': 20520,                             # 513*4*8 + 513*8
    'cdft_lds(1638, 4)': 65520,                            # 1638*4*8 + 1638*8
    'cdft_lds(1639, 4)': 65560,                            # 1639*4*8 + 1639*8
    'irdft_off_cos_f(129)': 258,                           # 2*129
    'irdft_off_sin_f(129, 256)': 514,                      # 2*129 + 256
    'irdft_lds(129, 256)': 3080,                           # 129*8 + 256*8
    'irdft_lds(2731, 5461)': 65536,                        # 2731*8 + 5461*8
    'irdft_lds(2732, 5462)': 65552,                        # 2732*8 + 5462*8
    'irdft_lds(2, 2)': 32,                                 # 2*8 + 2*8
    'irdft_lds(4097, 8192)': 98312,                        # 4097*8 + 8192*8
}

# (patch end, end of the area under it): every alias the kernels assert, evaluated on the host
ALIASES = [
    ("TM_TRB(36)", "TM_OFF_XL"),                          # token_mlp / token_projmlp epilogue patches inside the W images
    ("TM_TRB(33)", "TM_OFF_XL"),
    ("32 * FF_XS_ROW * 4", "32 * XLROWB"),                # a wave's row-gather patch inside its own x_lo rows
    ("W1PIECES * 1024", "2 * TM_W1B"),                    # token_projmlp's projection ring: slot 0 = the W1 area, slot 1 = the W2 area
    ("W1PIECES * 1024", "2 * TM_W2B"),
    ("PM_OFF_W2 + 2 * PM_W2SLOT", "PM_PROJB"),            # token_projmlp_bf16: the MLP ring over the projection image, below the patches
    ("ff_patches_bytes(8, 33)", "nffn_off_b4(4)"),        # naf_ffn epilogue patches below the b4 vector
    ("ff_patches_bytes(8, 33)", "nffn_off_b4(8)"),
    ("ff_patches_bytes(1, FF_XS_ROW)", "32 * nffn_xlrowb(8)"),   # naf_ffn, KS = 8: the gather patch inside the wave's x_lo rows
    ("WAB_OFF_TOKQ + 8 * 32 * 4", "WAB_OFF_KTOK"),        # attention_bf16: transposes + query rows inside the K / V staging
    ("ff_patches_bytes(8, 36)", "gemm_lds(128, 64, cig_rowb(32))"),   # smallest 8-wave ring of conv_igemm_bf16
    ("ff_patches_bytes(8, 36)", "gemm_lds(128, 64, RG_ROWB)"),        # and of gemm_rows_bf16
]


# every instantiation of launch_halo<WM, WN, MI, NI, WK, NSLOT, NTERMS> (conv3x3_halo.hip's dispatch) and every (BM, BN, row bytes, waves) of
# conv_gemm_bf16.hip's cfg 1 .. 9 and gemm_rows_bf16.hip's cfg 1, 2
HALO = ["8,1,1,2,64,9,1", "4,1,1,1,64,2,1", "8,1,1,1,64,2,3", "8,1,1,1,64,2,1", "8,1,1,2,64,2,3", "8,1,1,2,64,2,1", "2,2,2,2,64,2,3", "2,2,2,2,64,2,1",
        "4,2,2,3,32,2,3", "4,2,2,3,32,2,1"]
GEMM_CFGS = ["128, 128, cig_rowb(32), 4", "128, 64, cig_rowb(32), 4", "256, 32, cig_rowb(32), 4", "256, 192, cig_rowb(32), 8", "128, 128, cig_rowb(32), 8",
             "256, 128, cig_rowb(32), 8", "128, 64, cig_rowb(32), 8", "128, 128, cig_rowb(64), 8", "128, 64, cig_rowb(64), 8", "128, 128, RG_ROWB, 8",
             "128, 64, RG_ROWB, 8"]


@pytest.fixture(scope="module")
def values(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lds_layout") / "lds_layout_shim")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "image-super-resolution-2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lds_layout_shim.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    return {k: int(v) for k, v in (ln.rsplit(" ", 1) for ln in r.stdout.splitlines())}


def test_offsets_and_launch_byte_counts_are_the_parents(values):
    wrong = {k: (values.get(k), v) for k, v in EXPECTED.items() if values.get(k) != v}
    assert not wrong, wrong


def test_the_issues_example():
    # ff_token_linear, kpad 192, n_tiles 17
    assert EXPECTED["tl_off_vec(12, 17, 1)"] == 51200 + 36864 + 69632 + 2176 == 159872


def test_edges_of_the_run_time_parameters():
    # the largest value that still fits and the first that does not, per run-time parameter
    for fits, over, limit in [("tl_off_vec(12, 48, 1)", "tl_off_vec(12, 49, 1)", LDS_MAX), ("tl_off_vec(4, 304, 1)", "tl_off_vec(4, 305, 1)", LDS_MAX),
                              ("tl_off_vec(8, 176, 1)", "tl_off_vec(8, 177, 1)", LDS_MAX), ("tl_off_vec(12, 24, 2)", "tl_off_vec(12, 25, 2)", LDS_MAX),
                              ("tl_lds(4, 152, 2)", "tl_lds(4, 153, 2)", LDS_MAX), ("tl_lds(8, 88, 2)", "tl_lds(8, 89, 2)", LDS_MAX),
                              ("rdft_lds(5461)", "rdft_lds(5462)", LDS_DEFAULT_MAX), ("irdft_lds(2731, 5461)", "irdft_lds(2732, 5462)", LDS_DEFAULT_MAX),
                              ("TM_LDS(40)", "TM_LDS(41)", LDS_MAX), ("PM_LDS(88)", "PM_LDS(89)", LDS_MAX),
                              ("wab_lds(3456, 0, false, false)", "wab_lds(3584, 0, false, false)", LDS_DEFAULT_MAX),
                              ("cdft_lds(481, 16)", "cdft_lds(482, 16)", LDS_DEFAULT_MAX), ("cdft_lds(1638, 4)", "cdft_lds(1639, 4)", LDS_DEFAULT_MAX)]:
        assert EXPECTED[fits] <= limit < EXPECTED[over], (fits, over)
    assert EXPECTED["c3s_lds(64)"] == 88128 <= LDS_MAX                   # ff_conv3x3_small accepts Cin <= 64 and raises its kernels to exactly this
    # the row transforms are launched without raising the limit and their entry points accept W up to 8192: above W = 5461 the launch
    # itself fails (as before the maps existed; recorded as a finding, not changed here)
    assert EXPECTED["rdft_lds(8192)"] == 98304 > LDS_DEFAULT_MAX and EXPECTED["irdft_lds(4097, 8192)"] == 98312 > LDS_DEFAULT_MAX
    # the fixed images fit
    for k in ("nffn_lds(4)", "nffn_lds(8)", "nfr_lds(64)", "nfr_lds(128)", "ntl_lds(4, 4, true)", "ntl_lds(8, 4, true)", "WF_LDS", "W2_LDS",
              "gemm_lds(256, 192, cig_rowb(32))", "gemm_lds(256, 128, cig_rowb(32))", "gemm_lds(128, 128, cig_rowb(32))", "gemm_lds(128, 128, cig_rowb(64))"):
        assert EXPECTED[k] <= LDS_MAX, k
    for inst in HALO:
        assert EXPECTED[f"halo<{inst}>.lds"] <= LDS_MAX, inst
    assert EXPECTED["halo<4,1,1,1,64,2,1>.lds"] == 38400 and EXPECTED["halo<4,2,2,3,32,2,3>.lds"] == 147456      # the smallest and the largest image
    for k in ("wat_lds(4)", "gemm_lds(128, 128, CG_LDK * 4)", "gemm_lds(256, 32, CG_LDK * 4)", "gemm_lds(128, 128, RG_ROWB)"):
        assert EXPECTED[k] <= LDS_DEFAULT_MAX, k


def test_both_branches_of_every_condition():
    e = EXPECTED
    assert e["nffn_lds(4)"] - e["nffn_off_xst(4)"] == 8 * 32 * 68 * 4 and e["nffn_lds(8)"] == e["nffn_off_xst(8)"]      # KS 4 / 8
    assert e["ntl_lds(4, 4, true)"] - e["ntl_lds(4, 4, false)"] == 4 * 64 * 4                                            # IMG
    assert e["ntl_lds(8, 4, true)"] - e["ntl_lds(8, 4, false)"] == 4 * 128 * 4
    assert e["wab_lds(256, 961, true, false)"] - e["wab_lds(256, 961, false, false)"] == 961 * 4                        # rel_table
    assert e["wab_lds(640, 1521, true, true)"] - e["wab_lds(640, 1521, false, false)"] == 1521 * 4 + 640 * 4            # + rel_gen
    assert e["tl_lds(12, 17, 2)"] - e["tl_lds(12, 17, 1)"] == 17 * 32 * 4                                                # rows16 against plain


@pytest.mark.parametrize("patch,area", ALIASES, ids=[f"{a} <= {b}" for a, b in ALIASES])
def test_every_patch_ends_inside_the_area_under_it(values, patch, area):
    assert values[patch] <= values[area], (values[patch], values[area])


@pytest.mark.parametrize("inst", HALO)
def test_halo_epilogues_fit_in_every_launched_image(values, inst):
    # the vector epilogue's pool row and patches, and the scalar epilogue's pool row, against the instantiation's own launch size
    assert values[f"halo<{inst}>.lds"] == EXPECTED[f"halo<{inst}>.lds"]
    assert values[f"halo<{inst}>.vec_epilogue_fits"] == 1 and values[f"halo<{inst}>.pool_row_fits"] == 1


@pytest.mark.parametrize("cfg", GEMM_CFGS)
def test_gemm_epilogue_patches_fit_in_every_launched_ring(values, cfg):
    assert values[f"gemm_patches_fit({cfg})"] == 1


def test_alias_predicates(values):
    assert values["gemm_patches_fit(64, 32, RG_ROWB, 8)"] == 0          # 24 576 B of ring under 36 864 B of patches: must say no
    assert values["halo_epilogue_fits(4, 1, 32, 38400)"] == 1           # the smallest launched image, <4,1,1,1,64,2,1>
    assert values["halo_epilogue_fits(4, 1, 32, 8192 + 18431)"] == 0    # one byte short of its four patches
    assert values["halo_epilogue_fits(8, 1, 288, 163840)"] == 0         # a pool row of 9 216 B would reach over HALO_OFF_PATCH
    # naf_ffn at KS = 4: the gather patch does NOT fit in the x_lo rows, which is why that form has staging patches of its own
    assert values["ff_patches_bytes(1, FF_XS_ROW)"] > values["32 * nffn_xlrowb(4)"] and EXPECTED["nffn_xs_in_xl(4)"] == 0


# ---- the over-limit side, through the entry points: refused before any launch -------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from isr2_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def ptr():
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    yield p
    del buf


def _refused(L, rc, who, msg):
    err = L.ff_last_error()
    assert rc == 1 and who in err and msg in err, (rc, err)              # FF_ERR_ARG


def test_token_linear_refuses_the_first_n_tiles_over_the_limit(L, ptr):
    p = ptr
    assert EXPECTED["tl_off_vec(12, 49, 1)"] > LDS_MAX
    rc = L.ff_token_linear(p, 192, p, 1568, 256, 192, 192, 1568, 49, None, None, 1e-5, p, None, 0, None, 0, None, 0, None, None, 0, None, 0, 0, 0.0, 3, None)
    _refused(L, rc, b"ff_token_linear:", b"N too large for the LDS image")


def test_token_linear_rows16_refuses_the_first_n_tiles_over_the_limit(L, ptr):
    p = ptr
    assert EXPECTED["tl_off_vec(12, 25, 2)"] > LDS_MAX
    rc = L.ff_token_linear_rows16(p, 192, p, 800, 256, 192, 192, 800, 25, None, None, 1e-5, p, None, p, 0, None, 0, None, 0, None, None, 0, None, 0, 0, 0.0,
                                  1, None)
    _refused(L, rc, b"ff_token_linear_rows16:", b"N too large for the LDS image")


def test_token_linear_gated_refuses_the_first_n_tiles_over_the_limit(L, ptr):
    p = ptr
    rc = L.ff_token_linear_gated(p, 192, p, 192, p, p, p, p, 0.0, p, 1568, 256, 192, 1568, 49, p, None, None, 0, 3, None)
    _refused(L, rc, b"ff_token_linear_gated:", b"N too large for the LDS image")


@pytest.mark.parametrize("nterms", [3, 1])
def test_token_mlp_refuses_the_first_hidden_tile_over_the_limit(L, ptr, nterms):
    p = ptr
    assert EXPECTED["TM_LDS(41)"] > LDS_MAX
    rc = L.ff_token_mlp(p, 192, p, 192, 256, 180, 41, 180, p, p, 1e-5, p, p, p, nterms, None)
    _refused(L, rc, b"ff_token_mlp:", b"hidden too large for the LDS image")


@pytest.mark.parametrize("nterms", [3, 1])
def test_token_projmlp_refuses_the_first_hidden_tile_over_the_limit(L, ptr, nterms):
    p = ptr
    rc = L.ff_token_projmlp(p, 192, p, 192, None, 0, None, p, 192, 256, 180, 41, p, p, p, p, 1e-5, p, p, p, nterms, 0, None)
    _refused(L, rc, b"ff_token_projmlp:", b"hidden too large for the LDS image")


def test_window_attn_bf16_refuses_a_key_window_over_the_default_limit(L, ptr):
    p = ptr
    assert 37888 + 2 * 4096 * 4 > LDS_DEFAULT_MAX                       # 64 x 64 keys: nkpad 4096, no tables
    rc = L.ff_window_attn_bf16s(p, 540, 0, 180, 360, p, 180, 0, p, 1, 64, 64, 64, 64, 16, 16, 64, 64, 0, 0, 0, 6, 30, 0.18, 3, None, None)
    _refused(L, rc, b"ff_window_attn_bf16s:", b"window too large for the LDS image")
