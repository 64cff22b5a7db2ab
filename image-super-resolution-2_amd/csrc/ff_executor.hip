// C-level executor: replays a launch plan recorded from the Python host (isr2_amd/plan.py) -- every kernel of
// CompleteEnhancedFusionSR.forward in eval mode (src/models/enhanced_fusion.py:694-754, the call the reference plugin makes at
// models/team29_FreqFusion/io.py:221) for one input shape -- without Python in the loop:
//     ff_create(plan) -> ff_upload(slot, bytes) for every prepared-weight slot -> ff_finalize -> ff_forward(lr, out, stream) ...
// The library owns its weight copies and one workspace (packed by buffer lifetime at export time); the caller owns the input
// and output tensors; every launch goes to the caller's stream in plan order, so ff_forward is asynchronous and
// graph-capturable like the per-operator entry points it drives.  No internal threads; one handle per host thread.
// ff_forward_image_u8 serves images of any size at least the tile's from ONE tile plan: uint8 in, overlap tiles B at a time, uint8 out.
// ff_forward_image_ens_u8 is its x8 geometric self-ensemble: the same loop once per symmetry, folded into one fp32 accumulator.
#include "ff_common.h"
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include <vector>

extern "C" int ff_abi_version(void);
extern "C" int ff_tile_positions(int n, int tile, int step, int* out, int cap);      // csrc/tile_image.hip (pure host)
union FFVal { long long i; double f; void* p; };
#include "ff_dispatch_gen.h"      // generated from include/ff_kernels.h by build.py: FF_DISPATCH_NAMES[], ff_dispatch(id, vals)

enum { K_INT = 0, K_FLT, K_NULL, K_WEIGHT, K_WORK, K_INPUT, K_OUTPUT, K_STREAM };

struct PlanArg { uint8_t kind; long long a, b; double f; };
struct PlanCall { int fn; int first, n; int stream; };      // fn == -1: fork (stream 0) / join (stream 1) marker
struct PlanSlot { std::string name; long long nbytes; void* dev; bool filled; };
struct ff_model {
  std::vector<PlanSlot> slots;
  std::vector<PlanCall> calls;
  std::vector<PlanArg> args;
  long long wbytes = 0;
  void* work = nullptr;
  int in[4], out[4];
  bool finalized = false;
  // the host's three-stream schedule: between a fork and a join marker the launches of stream 1 / 2 go to two internal streams
  hipStream_t side[2] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
  int nstreams = 1;
};

static bool rd(FILE* f, void* dst, size_t n) { return fread(dst, 1, n, f) == n; }

static void free_model(ff_model* m) {
  if (!m) return;
  for (auto& s : m->slots) if (s.dev) (void)hipFree(s.dev);
  if (m->work) (void)hipFree(m->work);
  for (int i = 0; i < 2; ++i) { if (m->side[i]) (void)hipStreamDestroy(m->side[i]); if (m->ev_join[i]) (void)hipEventDestroy(m->ev_join[i]); }
  if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
  delete m;
}

extern "C" int ff_create(const char* plan_path, void** out_handle) {
  FF_CHECK_ARG(plan_path && out_handle, "ff_create: null argument");
  *out_handle = nullptr;
  FILE* f = fopen(plan_path, "rb");
  FF_CHECK_ARG(f, "ff_create: cannot open %s", plan_path);
  ff_model* m = new ff_model();
  auto fail = [&](const char* why) { ff_set_error("ff_create: %s: %s", plan_path, why); fclose(f); free_model(m); return FF_ERR_ARG; };
  char magic[8];
  int32_t abi; uint32_t nnames;
  if (!rd(f, magic, 8) || memcmp(magic, "FFPLAN3\0", 8) != 0) return fail("not an FFPLAN3 file");
  if (!rd(f, &abi, 4) || !rd(f, &nnames, 4) || nnames > 4096) return fail("truncated header");
  if (abi != ff_abi_version()) return fail("plan was recorded against another ABI version of the kernel library");
  std::vector<int> fnmap(nnames, -1);
  for (uint32_t i = 0; i < nnames; ++i) {
    uint32_t ln;
    if (!rd(f, &ln, 4) || ln > 256) return fail("bad entry-point name");
    std::string nm(ln, '\0');
    if (!rd(f, &nm[0], ln)) return fail("truncated names");
    for (int k = 0; k < FF_DISPATCH_COUNT; ++k)
      if (nm == FF_DISPATCH_NAMES[k]) fnmap[i] = k;
    if (fnmap[i] < 0) { ff_set_error("ff_create: %s uses entry point %s, which this library does not export", plan_path, nm.c_str()); fclose(f); free_model(m); return FF_ERR_ARG; }
  }
  uint32_t nslots;
  if (!rd(f, &nslots, 4) || nslots > (1u << 20)) return fail("bad slot count");
  m->slots.resize(nslots);
  for (auto& s : m->slots) {
    uint32_t ln;
    if (!rd(f, &ln, 4) || ln > 1024) return fail("bad slot name");
    s.name.assign(ln, '\0');
    if (!rd(f, &s.name[0], ln) || !rd(f, &s.nbytes, 8) || s.nbytes < 0) return fail("truncated slot table");
    s.dev = nullptr; s.filled = false;
  }
  if (!rd(f, &m->wbytes, 8) || !rd(f, m->in, 16) || !rd(f, m->out, 16) || m->wbytes < 0) return fail("truncated shapes");
  uint32_t ncalls;
  if (!rd(f, &ncalls, 4) || ncalls > (1u << 24)) return fail("bad call count");
  m->calls.resize(ncalls);
  for (auto& c : m->calls) {
    uint16_t fid, na, sid;
    if (!rd(f, &fid, 2) || !rd(f, &na, 2) || !rd(f, &sid, 2)) return fail("bad call record");
    if (fid == 0xFFFF) { c.fn = -1; c.first = 0; c.n = 0; c.stream = sid; if (sid > 1) return fail("bad marker"); continue; }
    if (fid >= nnames || na > 64 || sid > 2) return fail("bad call record");
    c.fn = fnmap[fid]; c.first = (int)m->args.size(); c.n = na; c.stream = sid;
    const char* kinds = FF_DISPATCH_KINDS[c.fn];
    if ((size_t)na != strlen(kinds)) { ff_set_error("ff_create: %s: a call of %s carries %d arguments, the entry point takes %zu", plan_path, FF_DISPATCH_NAMES[c.fn], (int)na, strlen(kinds)); fclose(f); free_model(m); return FF_ERR_ARG; }
    if (sid + 1 > m->nstreams) m->nstreams = sid + 1;
    for (int i = 0; i < na; ++i) {
      unsigned char rec[20];
      if (!rd(f, rec, 20)) return fail("truncated arguments");
      PlanArg a; a.kind = rec[0]; a.a = 0; a.b = 0; a.f = 0.0;
      if (a.kind == K_FLT) memcpy(&a.f, rec + 4, 8);
      else { memcpy(&a.a, rec + 4, 8); memcpy(&a.b, rec + 12, 8); }
      if (a.kind > K_STREAM) return fail("bad argument kind");
      if (a.kind == K_WEIGHT && (a.a < 0 || a.a >= (long long)nslots || a.b < 0 || a.b >= m->slots[a.a].nbytes)) return fail("weight reference out of range");
      if (a.kind == K_WORK && (a.b < 0 || a.b >= m->wbytes)) return fail("workspace reference out of range");
      {
        const long long in_bytes = 4LL * m->in[0] * m->in[1] * m->in[2] * m->in[3], out_bytes = 4LL * m->out[0] * m->out[1] * m->out[2] * m->out[3];
        if (a.kind == K_INPUT && (a.b < 0 || a.b >= in_bytes)) return fail("input reference beyond the lr tensor");
        if (a.kind == K_OUTPUT && (a.b < 0 || a.b >= out_bytes)) return fail("output reference beyond the sr tensor");
        const char want = kinds[i];
        const bool ok = want == 'P' ? (a.kind == K_NULL || a.kind == K_WEIGHT || a.kind == K_WORK || a.kind == K_INPUT || a.kind == K_OUTPUT)
                       : want == 'I' ? a.kind == K_INT : want == 'F' ? a.kind == K_FLT : a.kind == K_STREAM;
        if (!ok) { ff_set_error("ff_create: %s: argument %d of %s has kind %d where the prototype has '%c'", plan_path, i, FF_DISPATCH_NAMES[c.fn], (int)a.kind, want); fclose(f); free_model(m); return FF_ERR_ARG; }
      }
      m->args.push_back(a);
    }
  }
  fclose(f);
  for (auto& s : m->slots)
    if (hipMalloc(&s.dev, (size_t)(s.nbytes > 0 ? s.nbytes : 1)) != hipSuccess) { ff_set_error("ff_create: hipMalloc of slot %s (%lld bytes) failed", s.name.c_str(), s.nbytes); free_model(m); return FF_ERR_LAUNCH; }
  if (hipMalloc(&m->work, (size_t)(m->wbytes > 0 ? m->wbytes : 1)) != hipSuccess) { ff_set_error("ff_create: hipMalloc of the %lld-byte workspace failed", m->wbytes); free_model(m); return FF_ERR_LAUNCH; }
  if (m->nstreams > 1) {
    bool ok = hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && ok; ++i)
      ok = hipStreamCreateWithFlags(&m->side[i], hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&m->ev_join[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) { ff_set_error("ff_create: cannot create the executor's streams / events"); free_model(m); return FF_ERR_LAUNCH; }
  }
  *out_handle = m;
  return FF_OK;
}

extern "C" int ff_upload(void* handle, const char* slot_name, const void* host_or_dev_ptr, long long nbytes) {
  ff_model* m = (ff_model*)handle;
  FF_CHECK_ARG(m && slot_name && host_or_dev_ptr, "ff_upload: null argument");
  for (auto& s : m->slots)
    if (s.name == slot_name) {
      FF_CHECK_ARG(nbytes == s.nbytes, "ff_upload: slot %s holds %lld bytes, got %lld", slot_name, s.nbytes, nbytes);
      if (hipMemcpy(s.dev, host_or_dev_ptr, (size_t)nbytes, hipMemcpyDefault) != hipSuccess) { ff_set_error("ff_upload: copy into %s failed", slot_name); return FF_ERR_LAUNCH; }
      s.filled = true;
      return FF_OK;
    }
  ff_set_error("ff_upload: the plan has no slot named %s", slot_name);
  return FF_ERR_ARG;
}

extern "C" int ff_finalize(void* handle) {
  ff_model* m = (ff_model*)handle;
  FF_CHECK_ARG(m, "ff_finalize: null handle");
  for (auto& s : m->slots) FF_CHECK_ARG(s.filled, "ff_finalize: slot %s was never uploaded", s.name.c_str());
  m->finalized = true;
  return FF_OK;
}

// One replay of the plan: lr_dev / out_dev stand for the plan's input / output space.  `who` names the entry point in a fork / join error.
static int replay_plan(ff_model* m, const float* lr_dev, float* out_dev, void* stream, const char* who) {
  FFVal v[64];
  hipStream_t main_st = (hipStream_t)stream;
  for (const PlanCall& c : m->calls) {
    if (c.fn < 0) {
      if (m->nstreams > 1) {
        bool ok = true;
        if (c.stream == 0) {                                 // fork: the side streams wait for everything issued on the caller's stream so far
          ok = hipEventRecord(m->ev_fork, main_st) == hipSuccess;
          for (int i = 0; i < 2 && ok; ++i) ok = hipStreamWaitEvent(m->side[i], m->ev_fork, 0) == hipSuccess;
        } else {                                             // join: the caller's stream waits for both side streams
          for (int i = 0; i < 2 && ok; ++i)
            ok = hipEventRecord(m->ev_join[i], m->side[i]) == hipSuccess && hipStreamWaitEvent(main_st, m->ev_join[i], 0) == hipSuccess;
        }
        if (!ok) { ff_set_error("%s: stream fork / join failed: %s", who, hipGetErrorString(hipGetLastError())); return FF_ERR_LAUNCH; }
      }
      continue;
    }
    void* call_stream = (c.stream == 0 || m->nstreams == 1) ? stream : (void*)m->side[c.stream - 1];
    for (int i = 0; i < c.n; ++i) {
      const PlanArg& a = m->args[c.first + i];
      switch (a.kind) {
        case K_INT: v[i].i = a.a; break;
        case K_FLT: v[i].f = a.f; break;
        case K_NULL: v[i].p = nullptr; break;
        case K_WEIGHT: v[i].p = (char*)m->slots[a.a].dev + a.b; break;
        case K_WORK: v[i].p = (char*)m->work + a.b; break;
        case K_INPUT: v[i].p = (char*)lr_dev + a.b; break;
        case K_OUTPUT: v[i].p = (char*)out_dev + a.b; break;
        default: v[i].p = call_stream; break;
      }
    }
    const int rc = ff_dispatch(c.fn, v);
    if (rc != FF_OK) return rc;               // ff_last_error() carries the failing entry point's message
  }
  return FF_OK;
}

extern "C" int ff_forward(void* handle, const float* lr_dev, int B, int H, int W, float* out_dev, void* stream) {
  ff_model* m = (ff_model*)handle;
  FF_CHECK_ARG(m && lr_dev && out_dev, "ff_forward: null argument");
  FF_CHECK_ARG(m->finalized, "ff_forward: ff_finalize has not succeeded on this handle");
  FF_CHECK_ARG(B == m->in[0] && H == m->in[2] && W == m->in[3], "ff_forward: this plan is for input [%d,3,%d,%d], got [%d,3,%d,%d]", m->in[0], m->in[2], m->in[3], B, H, W);
  return replay_plan(m, lr_dev, out_dev, stream, "ff_forward");
}

// ---- any-size images through a TILE plan ([B,3,t,t] -> [B,3,4t,4t], B <= 16): the plugin's _tiled_forward (models/team29_FreqFusion/
// io.py:116-164) on uint8 images, B tiles per replay.  The caller's work buffer, every part 256-byte aligned, in this order:
//     acc [3][4H][4W] fp32 | wsum [4H][4W] fp32 | tile input [B,3,t,t] fp32 | tile output [B,3,4t,4t] fp32 | ramp table [4][4t] fp32
// After the call acc and wsum hold the un-normalised canvas (ff_tile_finish_u8 only reads them).
enum { IW_ACC = 0, IW_WSUM, IW_TIN, IW_TOUT, IW_RAMPS, IW_PARTS };
static const int IMAGE_SCALE = 4, IMAGE_MAX_BATCH = 16;

static bool tile_plan_ok(const ff_model* m) {
  const int* a = m->in; const int* b = m->out;
  return a[0] >= 1 && a[0] <= IMAGE_MAX_BATCH && a[1] == 3 && a[2] >= 1 && a[2] == a[3] && b[0] == a[0] && b[1] == 3 &&
         b[2] == IMAGE_SCALE * a[2] && b[3] == IMAGE_SCALE * a[3];
}

static long long image_layout(const ff_model* m, int H, int W, long long (&off)[IW_PARTS]) {
  const long long B = m->in[0], t = m->in[2], P = (long long)IMAGE_SCALE * H * IMAGE_SCALE * W, st = IMAGE_SCALE * t;
  const long long bytes[IW_PARTS] = {12 * P, 4 * P, 12 * B * t * t, 12 * B * st * st, 16 * st};
  long long at = 0;
  for (int i = 0; i < IW_PARTS; ++i) { off[i] = at; at += (bytes[i] + 255) / 256 * 256; }
  return at;
}

// what the two workspace queries refuse (with a message that names `who`): a null handle, a plan that is no tile plan, an image smaller than the tile
static bool workspace_query_ok(const ff_model* m, int H, int W, const char* who) {
  if (!m) { ff_set_error("%s: null handle", who); return false; }
  if (!tile_plan_ok(m)) { ff_set_error("%s: not a tile plan (input [%d,%d,%d,%d], output [%d,%d,%d,%d])", who, m->in[0], m->in[1], m->in[2], m->in[3], m->out[0], m->out[1], m->out[2], m->out[3]); return false; }
  if (H < m->in[2] || W < m->in[3]) { ff_set_error("%s: a %dx%d image is smaller than the plan's %dx%d tile", who, H, W, m->in[2], m->in[3]); return false; }
  return true;
}

extern "C" long long ff_image_workspace_bytes(void* handle, int H, int W) {
  ff_model* m = (ff_model*)handle;
  if (!workspace_query_ok(m, H, W, "ff_image_workspace_bytes")) return -1;
  long long off[IW_PARTS];
  return image_layout(m, H, W, off);
}

// The checks the two image entry points share, in ff_forward_image_u8's order and wording; `who` names the entry point.
static int image_args_ok(const ff_model* m, int H, int W, int overlap, const char* who) {
  FF_CHECK_ARG(m->finalized, "%s: ff_finalize has not succeeded on this handle", who);
  FF_CHECK_ARG(tile_plan_ok(m), "%s: the handle's plan must map square tiles [B,3,t,t] to [B,3,4t,4t] with B <= %d; this one maps [%d,%d,%d,%d] to [%d,%d,%d,%d]",
               who, IMAGE_MAX_BATCH, m->in[0], m->in[1], m->in[2], m->in[3], m->out[0], m->out[1], m->out[2], m->out[3]);
  const int t = m->in[2];
  FF_CHECK_ARG(H <= (1 << 28) && W <= (1 << 28), "%s: a %dx%d image is beyond the 2^28 samples per side that 4H and 4W as int allow", who, H, W);
  FF_CHECK_ARG(H >= t && W >= t, "%s: a %dx%d image does not hold one full %dx%d tile of this plan (ragged tiles, as the reference "
               "cuts from images smaller than the tile, are out of scope)", who, H, W, t, t);
  FF_CHECK_ARG(overlap >= 0 && overlap < t, "%s: overlap %d must lie in [0, tile = %d)", who, overlap, t);
  return FF_OK;
}

// The canvas of ONE image from its tiles, the loop both image entry points run: clear acc and wsum, (write the ramp table,) then per
// group of B tiles B cuts, one replay and one ff_tile_accum per real tile in tile order.  The image the tiles are cut from is
// T_code(img), Ht x Wt, with ys / xs its tile origins; code < 0 is the plain image through ff_tile_cut_u8 (ff_forward_image_u8's
// launches), code >= 0 goes through ff_tile_cut_u8_d4 and never materialises T_code(img).  Rows of the ramp table are chosen from
// the TRANSFORMED image's neighbours, as _tiled_forward would on d4_rect(lr, code).
static int canvas_from_tiles(ff_model* m, const unsigned char* img_dev, int H, int W, int code, int overlap, const std::vector<int>& ys,
                             const std::vector<int>& xs, void* work, const long long (&off)[IW_PARTS], bool write_ramps, void* stream,
                             const char* who) {
  const int B = m->in[0], t = m->in[2], st = IMAGE_SCALE * t;
  const int odd = code >= 0 && ((code >> 2) & 1);
  const int Ht = odd ? W : H, Wt = odd ? H : W;
  const int blend = IMAGE_SCALE * overlap < st / 4 ? IMAGE_SCALE * overlap : st / 4;
  const int nx = (int)xs.size();
  float* acc = (float*)((char*)work + off[IW_ACC]);
  float* wsum = (float*)((char*)work + off[IW_WSUM]);
  float* tin = (float*)((char*)work + off[IW_TIN]);
  float* tout = (float*)((char*)work + off[IW_TOUT]);
  float* tab = (float*)((char*)work + off[IW_RAMPS]);
  const int HS = IMAGE_SCALE * Ht, WS = IMAGE_SCALE * Wt;
  const long long P = (long long)HS * WS;
  if (hipMemsetAsync(acc, 0, (size_t)(12 * P), (hipStream_t)stream) != hipSuccess || hipMemsetAsync(wsum, 0, (size_t)(4 * P), (hipStream_t)stream) != hipSuccess) {
    ff_set_error("%s: clearing the canvas failed: %s", who, hipGetErrorString(hipGetLastError()));
    return FF_ERR_LAUNCH;
  }
  int rc = write_ramps ? ff_tile_ramps(tab, st, blend, stream) : FF_OK;
  if (rc != FF_OK) return rc;
  const long long ntiles = (long long)ys.size() * nx;
  for (long long g0 = 0; g0 < ntiles; g0 += B) {
    for (int s = 0; s < B; ++s) {                            // a short last group repeats its last tile: the forward reads no stale slot
      const long long k = g0 + s < ntiles ? g0 + s : ntiles - 1;
      float* slot = tin + (long long)s * 3 * t * t;
      rc = code < 0 ? ff_tile_cut_u8(img_dev, H, W, ys[k / nx], xs[k % nx], t, t, slot, stream)
                    : ff_tile_cut_u8_d4(img_dev, H, W, code, ys[k / nx], xs[k % nx], t, t, slot, stream);
      if (rc != FF_OK) return rc;
    }
    rc = replay_plan(m, tin, tout, stream, who);
    if (rc != FF_OK) return rc;
    for (int s = 0; s < B && g0 + s < ntiles; ++s) {         // in tile order (y outer, x inner), as the plugin accumulates
      const int y = ys[(g0 + s) / nx], x = xs[(g0 + s) % nx];
      const float* wy = tab + (long long)((y > 0 ? 1 : 0) + (y + t < Ht ? 2 : 0)) * st;
      const float* wx = tab + (long long)((x > 0 ? 1 : 0) + (x + t < Wt ? 2 : 0)) * st;
      rc = ff_tile_accum(tout + (long long)s * 3 * st * st, 3, st, st, wy, wx, acc, wsum, HS, WS, IMAGE_SCALE * y, IMAGE_SCALE * x, stream);
      if (rc != FF_OK) return rc;
    }
  }
  return FF_OK;
}

// the tile origins along an axis of n samples (ff_tile_positions into a vector); empty when they cannot be placed
static std::vector<int> axis_positions(int n, int t, int step) {
  std::vector<int> p((n - t) / step + 2);
  const int cnt = ff_tile_positions(n, t, step, p.data(), (int)p.size());
  p.resize(cnt > 0 ? cnt : 0);
  return p;
}

extern "C" int ff_forward_image_u8(void* handle, const unsigned char* img_dev, int H, int W, int overlap, unsigned char* out_dev, void* work,
                                   long long work_bytes, void* stream) {
  static const char* const who = "ff_forward_image_u8";
  ff_model* m = (ff_model*)handle;
  FF_CHECK_ARG(m && img_dev && out_dev && work, "ff_forward_image_u8: null argument");
  int rc = image_args_ok(m, H, W, overlap, who);
  if (rc != FF_OK) return rc;
  const int t = m->in[2], step = t - overlap;
  long long off[IW_PARTS];
  const long long need = image_layout(m, H, W, off);
  FF_CHECK_ARG(work_bytes >= need, "ff_forward_image_u8: a %dx%d image needs %lld bytes of work space, got %lld", H, W, need, work_bytes);
  const std::vector<int> ys = axis_positions(H, t, step), xs = axis_positions(W, t, step);
  FF_CHECK_ARG(!ys.empty() && !xs.empty(), "ff_forward_image_u8: cannot place %dx%d tiles with step %d on a %dx%d image", t, t, step, H, W);
  rc = canvas_from_tiles(m, img_dev, H, W, -1, overlap, ys, xs, work, off, true, stream, who);
  if (rc != FF_OK) return rc;
  return ff_tile_finish_u8((const float*)((char*)work + off[IW_ACC]), (const float*)((char*)work + off[IW_WSUM]), IMAGE_SCALE * H,
                           IMAGE_SCALE * W, out_dev, stream);
}

// ---- the x8 geometric self-ensemble of an image through the same tile plan (model.FreqFusionHIP.self_ensemble with
// run = _tiled_forward): per code the canvas of T_code(img) from canvas_from_tiles, then ONE ff_tile_fold_d4 that normalises it, maps it
// back by the inverse code and folds it into ens.  `work` = the parts of ff_forward_image_u8 for an H x W image (a W x H canvas has
// the same element count) followed by ens [3][4H][4W] fp32, which starts on a multiple of 256 bytes.
static long long image_ens_layout(const ff_model* m, int H, int W, long long (&off)[IW_PARTS], long long& ens_off) {
  ens_off = image_layout(m, H, W, off);                      // every part is padded to 256 bytes, so is their sum
  const long long P = (long long)IMAGE_SCALE * H * IMAGE_SCALE * W;
  return ens_off + (12 * P + 255) / 256 * 256;
}

// ops.d4_inverse_code / ops.d4_canonical_code: exactly one flip = a reflection, its own inverse; otherwise a rotation, k' = (4 - k) % 4.
// A half turn is both flips, so codes 8..15 name the symmetries of 0..7: toggle both flips and keep k - 2.
static int d4_inverse_code(int c) { return (c & 1) != ((c >> 1) & 1) ? c : (c & 3) | (((4 - (c >> 2)) % 4) << 2); }
static int d4_canonical_code(int c) { return c < 8 ? c : ((c & 3) ^ 3) | (((c >> 2) - 2) << 2); }

extern "C" long long ff_image_ens_workspace_bytes(void* handle, int H, int W) {
  ff_model* m = (ff_model*)handle;
  if (!workspace_query_ok(m, H, W, "ff_image_ens_workspace_bytes")) return -1;
  long long off[IW_PARTS], ens_off;
  return image_ens_layout(m, H, W, off, ens_off);
}

extern "C" int ff_forward_image_ens_u8(void* handle, const unsigned char* img_dev, int H, int W, int overlap, const int* codes, int ncodes,
                                       unsigned char* out_dev, void* work, long long work_bytes, void* stream) {
  static const char* const who = "ff_forward_image_ens_u8";
  ff_model* m = (ff_model*)handle;
  FF_CHECK_ARG(m && img_dev && codes && out_dev && work, "ff_forward_image_ens_u8: null argument");
  int rc = image_args_ok(m, H, W, overlap, who);             // H >= t and W >= t: both orientations hold a full tile
  if (rc != FF_OK) return rc;
  FF_CHECK_ARG(ncodes >= 1, "ff_forward_image_ens_u8: ncodes = %d, at least one symmetry code is needed", ncodes);
  for (int i = 0; i < ncodes; ++i) {
    FF_CHECK_ARG(codes[i] >= 0 && codes[i] < 16, "ff_forward_image_ens_u8: codes[%d] = %d outside 0..15 (bit 0 hflip, bit 1 vflip, bits 2-3 rot90 k)", i, codes[i]);
    for (int j = 0; j < i; ++j)
      FF_CHECK_ARG(d4_canonical_code(codes[j]) != d4_canonical_code(codes[i]),
                   "ff_forward_image_ens_u8: codes[%d] = %d and codes[%d] = %d name the same symmetry (codes 8..15 repeat 0..7)", j, codes[j], i, codes[i]);
  }
  const int t = m->in[2], step = t - overlap;
  long long off[IW_PARTS], ens_off;
  const long long need = image_ens_layout(m, H, W, off, ens_off);
  FF_CHECK_ARG(work_bytes >= need, "ff_forward_image_ens_u8: the ensemble of a %dx%d image needs %lld bytes of work space, got %lld", H, W, need, work_bytes);
  const std::vector<int> pH = axis_positions(H, t, step), pW = axis_positions(W, t, step);
  FF_CHECK_ARG(!pH.empty() && !pW.empty(), "ff_forward_image_ens_u8: cannot place %dx%d tiles with step %d on a %dx%d image", t, t, step, H, W);

  const float* acc = (const float*)((char*)work + off[IW_ACC]);
  const float* wsum = (const float*)((char*)work + off[IW_WSUM]);
  float* ens = (float*)((char*)work + ens_off);
  for (int i = 0; i < ncodes; ++i) {
    const int odd = (codes[i] >> 2) & 1;                     // odd k: T(img) is W x H, its rows are placed like the image's columns
    rc = canvas_from_tiles(m, img_dev, H, W, codes[i], overlap, odd ? pW : pH, odd ? pH : pW, work, off, i == 0, stream, who);
    if (rc != FF_OK) return rc;
    const float scale = i == ncodes - 1 ? (float)(1.0 / ncodes) : 1.0f;      // the double quotient narrowed once, as the Python host passes it
    rc = ff_tile_fold_d4(acc, wsum, IMAGE_SCALE * (odd ? W : H), IMAGE_SCALE * (odd ? H : W), d4_inverse_code(codes[i]), ens, i > 0, scale, stream);
    if (rc != FF_OK) return rc;
  }
  return ff_f32nchw_to_u8hwc(ens, out_dev, IMAGE_SCALE * H, IMAGE_SCALE * W, stream);
}

extern "C" int ff_destroy(void* handle) {
  free_model((ff_model*)handle);
  return FF_OK;
}

extern "C" int ff_model_io_shape(void* handle, int* in_shape4, int* out_shape4) {
  ff_model* m = (ff_model*)handle;
  FF_CHECK_ARG(m && in_shape4 && out_shape4, "ff_model_io_shape: null argument");
  for (int i = 0; i < 4; ++i) { in_shape4[i] = m->in[i]; out_shape4[i] = m->out[i]; }
  return FF_OK;
}
extern "C" int ff_model_num_slots(void* handle) { return handle ? (int)((ff_model*)handle)->slots.size() : -1; }
extern "C" const char* ff_model_slot_name(void* handle, int i) {
  ff_model* m = (ff_model*)handle;
  return (m && i >= 0 && i < (int)m->slots.size()) ? m->slots[i].name.c_str() : nullptr;
}
extern "C" long long ff_model_slot_bytes(void* handle, int i) {
  ff_model* m = (ff_model*)handle;
  return (m && i >= 0 && i < (int)m->slots.size()) ? m->slots[i].nbytes : -1;
}
extern "C" long long ff_model_workspace_bytes(void* handle) { return handle ? ((ff_model*)handle)->wbytes : -1; }
extern "C" int ff_model_num_launches(void* handle) { return handle ? (int)((ff_model*)handle)->calls.size() : -1; }
