// Phase timing of the persistent OCAB attention kernel (debug aid, not part of the product): 256 x 256 tokens, 6 heads.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -DFF_TIMING -Iimage-super-resolution-2_amd/csrc tools/oc_time.cpp -o tools/_dbg/oc_time
#include "../image-super-resolution-2_amd/csrc/ocab_attn.hip"
#include "phase_time.h"

int main() {
  const int H = 256, W = 256, C = 180; const long long M = (long long)H * W; const int ldq = 544;
  PtRand rnd{7};
  float* q = pt_upload(rnd.f32(M * ldq));
  float* rel = pt_upload(rnd.f32(6 * 1521));
  float* out = pt_zeros<float>(M * 192);
  auto run = [&]() { return ff_ocab_attn(q, ldq, 0, C, 2 * C, out, 192, 0, rel, 1, H, W, 6, 30, 16, 24, 0.1826f, 0, nullptr); };
  const char* names[64] = {}; names[0] = "start"; names[1] = "prologue (tables, stage 0)"; names[60] = "end";
  static char nb[64][40]; const char* ph[4] = {"next-stage loads issued", "9 tiles computed", "next stage stored", "barrier passed"};
  for (int n = 0; n < 4; ++n) for (int k = 0; k < 4; ++k) { snprintf(nb[2 + 4 * n + k], 40, "step %d %s", n, ph[k]); names[2 + 4 * n + k] = nb[2 + 4 * n + k]; }
  return pt_time_and_table("ocab_attn", run, 256 * 8, 64, names);
}
