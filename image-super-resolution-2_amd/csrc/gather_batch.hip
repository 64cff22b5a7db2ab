// One cached-expert micro-batch out of the resident sample pool (isr2_amd.epoch.ResidentCache / ResidentEpoch): the B samples a
// descriptor names are gathered and augmented -- lr, hr, the three expert images and the three feature maps -- in ONE launch.  The
// reference reads and augments each sample on the host before collation (src/data/cached_dataset.py:135-200, :240-268); CachedEpoch
// uploads the batch as read and permutes it with eight ff_d4_nchw launches (csrc/augment.hip).  Here nothing crosses the host.
//
//   pool    field-major fp32: field f is one contiguous [n_samples][C_f][H_f][W_f] array starting fields[f][0] floats into pool
//   fields  HOST int64 [F][5] = {pool_off, out_off, C, H, W}, read before the launch; 1 <= F <= 8
//   desc    DEVICE int32 [B][2] = {sample index, D4 code}: code = bit 0 hflip | bit 1 vflip | bits 2-3 k of rot90 (ff_d4_nchw's)
//   out     flat fp32: field f of the micro-batch is [B][C_f][H_f][W_f] starting at out + fields[f][1]
//
// One workgroup = one 64 x 64 OUTPUT tile of one plane of one field, moved by d4_tile<false> (csrc/d4_tile.inc, the body of
// d4_nchw_kernel): a pure copy, so NaN payloads, negative zero and denormals pass through.  The field table travels by value in the
// kernel arguments -- at most 8 entries, each with the index of its first workgroup -- and a workgroup finds its field by a uniform
// scan of that table: nothing diverges inside a workgroup, and no table is read from memory.  Every plane offset is 64-bit (a DF2K
// pool is 4.4e10 floats).  The 16-byte form is chosen per FIELD: W % 4 == 0 and both of the field's bases 16-byte aligned (then
// every plane of it is); any other field takes the dword form of the same loop.  No atomics.
// The sample index is clamped into [0, n_samples), the code is masked to 4 bits and its odd-turn bit is cleared on a non-square
// field (as d4_nchw_kernel does): ops.gather_d4_fields refuses such descriptors, and no descriptor can make the kernel read outside
// the pool.
#include "ff_common.h"

#include "d4_tile.inc"        // D4_TILE, D4_PITCH, d4_tile: the one body of every D4 kernel

#define GB_MAX_FIELDS 8

struct GatherField {
  long long pool_off, out_off;  // floats: first element of the field in the pool / in the flat output
  int C, H, W;
  int first_block;              // index of the field's first workgroup in the launch
  int tiles_x, tiles_per_plane;
  int vec4;                     // the field takes the 16-byte form
  int pad_;
};

struct GatherTable {
  GatherField f[GB_MAX_FIELDS];
};

__global__ __launch_bounds__(256) void gather_d4_fields_kernel(const float* __restrict__ pool, float* __restrict__ out,
                                                               const int* __restrict__ desc, long long n_samples, int F,
                                                               const GatherTable tab) {
  __shared__ float tile[D4_TILE * D4_PITCH];
  const int bid = (int)blockIdx.x;
  GatherField fd = tab.f[0];
#pragma unroll
  for (int i = 1; i < GB_MAX_FIELDS; ++i)                    // uniform scan: the last field that starts at or before this workgroup
    if (i < F && bid >= tab.f[i].first_block) fd = tab.f[i];
  const int r = bid - fd.first_block;
  const int plane = r / fd.tiles_per_plane, t = r - plane * fd.tiles_per_plane;    // plane of the micro-batch's field: b * C + c
  const int ty0 = (t / fd.tiles_x) * D4_TILE, tx0 = (t - (t / fd.tiles_x) * fd.tiles_x) * D4_TILE;      // origin of the OUTPUT tile
  const int b = plane / fd.C, c = plane - b * fd.C;
  long long idx = desc[2 * b];
  idx = idx < 0 ? 0 : (idx >= n_samples ? n_samples - 1 : idx);
  int code = desc[2 * b + 1] & 15;
  if (fd.H != fd.W) code &= ~4;                              // odd k on a non-square plane is refused by the host; never index outside
  const long long hw = (long long)fd.H * fd.W;
  d4_tile<false>(pool + fd.pool_off + (idx * fd.C + c) * hw, out + fd.out_off + (long long)plane * hw, tile, fd.H, fd.W, code, ty0, tx0,
                 fd.vec4, 0, 1.f);
}

extern "C" int ff_gather_d4_fields(const float* pool, long long n_samples, const long long* fields, int F, const int* desc, int B,
                                   float* out, void* stream) {
  FF_CHECK_ARG(pool && fields && desc && out, "ff_gather_d4_fields: null pointer");
  FF_CHECK_ARG(B >= 1 && F >= 1 && F <= GB_MAX_FIELDS && n_samples >= 1,
               "ff_gather_d4_fields: bad sizes (B %d and n_samples %lld must be >= 1, F %d in 1..%d)", B, n_samples, F, GB_MAX_FIELDS);
  GatherTable tab = {};
  long long blocks = 0;
  for (int i = 0; i < F; ++i) {
    const long long *fl = fields + 5 * i, C = fl[2], H = fl[3], W = fl[4];
    FF_CHECK_ARG(C >= 1 && H >= 1 && W >= 1 && C < (1ll << 31) && H < (1ll << 31) && W < (1ll << 31),
                 "ff_gather_d4_fields: field %d has shape C=%lld H=%lld W=%lld", i, C, H, W);
    FF_CHECK_ARG(fl[0] >= 0 && fl[1] >= 0, "ff_gather_d4_fields: field %d has negative offsets (pool %lld, out %lld)", i, fl[0], fl[1]);
    // the field's extent in the pool, and the end of it, are element offsets the kernel forms in 64 bits
    const __int128 ext = (__int128)n_samples * C * H * W + fl[0], oext = (__int128)B * C * H * W + fl[1];
    FF_CHECK_ARG(ext < ((__int128)1 << 61) && oext < ((__int128)1 << 61), "ff_gather_d4_fields: field %d does not fit 64-bit byte offsets", i);
    const int tiles_x = ff_cdiv(W, D4_TILE), tiles_y = ff_cdiv(H, D4_TILE);
    const __int128 upto = (__int128)B * C * tiles_x * tiles_y + blocks;
    FF_CHECK_ARG(upto < (1ll << 31), "ff_gather_d4_fields: the tiles of fields 0..%d exceed the grid limit of 2^31 - 1", i);
    GatherField& g = tab.f[i];
    g.pool_off = fl[0];
    g.out_off = fl[1];
    g.C = (int)C;
    g.H = (int)H;
    g.W = (int)W;
    g.first_block = (int)blocks;
    g.tiles_x = tiles_x;
    g.tiles_per_plane = tiles_x * tiles_y;
    g.vec4 = (W % 4 == 0) && (((uintptr_t)(pool + fl[0]) | (uintptr_t)(out + fl[1])) & 15) == 0;
    blocks = (long long)upto;
  }
  hipLaunchKernelGGL(gather_d4_fields_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pool, out, desc, n_samples, F, tab);
  FF_LAUNCH_CHECK("ff_gather_d4_fields");
  return FF_OK;
}
