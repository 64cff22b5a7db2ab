// Tile and LDS layout of the token MLP kernels (token_mlp.hip, hab_link.hip).
#pragma once
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
// ---- plain-bf16 form of token_projmlp
#define PM_W1SLOT (13 * 1024)
#define PM_W2SLOT (15 * 1024)
#define PM_OFF_W2 (2 * PM_W1SLOT)
#define PM_PROJB (6 * PM_W1SLOT)
#define PM_PATCHB (32 * FF_XS_ROW * 4)
#define PM_OFF_PATCH PM_PROJB
#define PM_OFF_VEC (PM_OFF_PATCH + 8 * PM_PATCHB)
