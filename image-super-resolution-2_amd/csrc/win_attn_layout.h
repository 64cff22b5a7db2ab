// LDS layout of the window-resident attention kernels (win_attn_fused.hip, win_attn_fused_v2.inc, hab_link.hip).
#pragma once
// ---- split-bf16 kernel (and the constants both forms share)
#define WF_KS 12
#define WF_SLOTS 25                        // 16-byte slots per weight row in LDS (24 data + 1 pad)
#define WF_ROWB (WF_SLOTS * 16)
#define WF_PL (32 * WF_SLOTS)              // slots per plane
#define WF_PLB (WF_PL * 16)                // bytes per plane
#define WF_BUFB (2 * WF_PLB)               // one ring slot (hi + lo) = 25 600 B = 25 DMA pieces
#define WF_TILE_ELEMS (32 * 192)
#define WF_KROWB 80
#define WF_KWAVE (2 * 32 * WF_KROWB)       // a wave's K rows, both planes: 5120 B (also its output transpose patch)
#define WF_VROWB 528
#define WF_VPLB (32 * WF_VROWB)
#define WF_OFF_K (2 * WF_BUFB)
#define WF_OFF_V (WF_OFF_K + 8 * WF_KWAVE)
#define WF_OFF_REL (WF_OFF_V + 2 * WF_VPLB)
#define WF_REL_MAX 2560                    // floats per head table (63 x 40 for the 32x8 window is the largest)
#define WF_REL_PAD 4                       // leading pad: keeps the lane part of the index non-negative
#define WF_OFF_BS (WF_OFF_REL + (WF_REL_MAX + WF_REL_PAD) * 4)
#define WF_BS_MAX 576
#define WF_OFF_TOK (WF_OFF_BS + WF_BS_MAX * 4)
#define WF_OFF_REG (WF_OFF_TOK + 1024)
#define WF_OFF_SAME (WF_OFF_REG + 1024)     // [9 regions][8 key tiles] 32-bit masks: which keys of the tile lie in the region
#define WF_LDS (WF_OFF_SAME + 9 * 8 * 4)
#define WF_XS_ROW 68
// ---- plain-bf16 form (win_attn_fused_v2.inc)
#define W2_TILEB (32 * WF_ROWB)                       // one 32-row weight tile, hi plane: 12 800 B
#define W2_HEAD_SLOTS (3 * WF_PL)                     // 16-byte slots of a head's q|k|v image
#define W2_PIECES ((W2_HEAD_SLOTS + 63) / 64)         // 1-KiB DMA pieces (38)
#define W2_WB (W2_PIECES * 1024)
#define W2_KROWB 80
#define W2_KWAVE (32 * W2_KROWB)
#define W2_KBUF (8 * W2_KWAVE)
#define W2_VROWB 528
#define W2_VBUF (32 * W2_VROWB)
#define W2_RELB ((WF_REL_MAX + WF_REL_PAD) * 4)
#define W2_OFF_K W2_WB
#define W2_OFF_V (W2_OFF_K + 2 * W2_KBUF)
#define W2_OFF_REL (W2_OFF_V + 2 * W2_VBUF)
#define W2_OFF_BS (W2_OFF_REL + 2 * W2_RELB)
#define W2_OFF_TOK (W2_OFF_BS + WF_BS_MAX * 4)
#define W2_OFF_REG (W2_OFF_TOK + 1024)
#define W2_OFF_SAME (W2_OFF_REG + 1024)
#define W2_LDS (W2_OFF_SAME + 9 * 8 * 4)
