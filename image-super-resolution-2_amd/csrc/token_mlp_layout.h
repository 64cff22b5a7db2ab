// Tile and LDS layout of the token MLP kernels (token_mlp.hip, hab_link.hip).
#pragma once
#include "lds_layout.h"   // FF_XS_ROW
#define TM_KP 192      // padded K (model dim 180)
#define TM_NP 192      // padded N
#define TM_KS 12       // k-steps of 16
#define W1SLOTS 25     // 16-byte slots per W1 row: 24 data (192 bf16) + 1 pad  -> 400 B
#define W2SLOTS 5      // slots per W2 row: 4 data (32 bf16) + 1 pad            -> 80 B
#define W1ROWB (W1SLOTS * 16)
#define W2ROWB (W2SLOTS * 16)
#define W1PL (32 * W1SLOTS)          // slots per W1 plane  (800)
#define W2PL (TM_NP * W2SLOTS)       // slots per W2 plane  (960)
#define W1PIECES (2 * W1PL / 64)      // 25
#define W2PIECES (2 * W2PL / 64)      // 30
#define TILE_ELEMS 6144              // bf16 elements per plane per hidden tile (32*192 == 192*32)
#define XLROWB 400                   // x_lo image row (per token): 192 bf16 + pad
// ---- split-bf16 kernels (token_mlp_kernel, token_projmlp_kernel): W1 [2 planes][32][400] | W2 [2 planes][192][80] |
// x_lo [8 waves][32 tokens][400] | b1 [ht * 32] floats.  ff_token_mlp and ff_token_projmlp both launch TM_LDS(hidden_tiles).
#define TM_W1B (W1PL * 16)
#define TM_W2B (W2PL * 16)
#define TM_OFF_W2 (2 * TM_W1B)
#define TM_OFF_XL (TM_OFF_W2 + 2 * TM_W2B)
#define TM_OFF_B1 (TM_OFF_XL + 8 * 32 * XLROWB)
#define TM_LDS(ht) ((size_t)TM_OFF_B1 + (size_t)(ht) * 32 * 4)
// what lies over what: a wave gathers its rows through its own (not yet written) x_lo rows; token_projmlp_kernel's projection ring
// uses the W1 and the W2 area as its two slots; the epilogues transpose through per-wave patches at the bottom of the idle W images
// (asserted at the pointers)
#define TM_TRB(row) (8 * 32 * (row) * 4)             // the eight waves' [32][row] float patches
static_assert(32 * FF_XS_ROW * 4 <= 32 * XLROWB, "token_mlp: a wave's gather patch must fit in its x_lo rows");
static_assert(W1PIECES * 1024 <= 2 * TM_W1B && W1PIECES * 1024 <= 2 * TM_W2B, "token_projmlp: a projection tile must fit in either W area");
// ---- plain-bf16 form of token_projmlp
#define PM_W1SLOT (13 * 1024)
#define PM_W2SLOT (15 * 1024)
#define PM_OFF_W2 (2 * PM_W1SLOT)
#define PM_PROJB (6 * PM_W1SLOT)
#define PM_PATCHB (32 * FF_XS_ROW * 4)
#define PM_OFF_PATCH PM_PROJB
#define PM_OFF_VEC (PM_OFF_PATCH + 8 * PM_PATCHB)
// token_projmlp_bf16_kernel's vectors from PM_OFF_VEC: gamma | beta | gate row | projection bias [TM_KP floats each] | b1 [ht * 32]
#define PM_OFF_BT (PM_OFF_VEC + TM_KP * 4)
#define PM_OFF_SC (PM_OFF_BT + TM_KP * 4)
#define PM_OFF_BP (PM_OFF_SC + TM_KP * 4)
#define PM_OFF_B1 (PM_OFF_BP + TM_KP * 4)
#define PM_LDS(ht) ((size_t)PM_OFF_B1 + (size_t)(ht) * 32 * 4)
static_assert(6 * 13 * 1024 <= PM_PROJB && PM_OFF_W2 + 2 * PM_W2SLOT <= PM_PROJB, "token_projmlp_bf16: the projection image, and the MLP ring laid over it, end below the patches");
