// Phase timing of the DAT SGFN tail (debug aid, not part of the product): 256 x 256 tokens, hidden 360, 180 outputs.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -DFF_TIMING -Iimage-super-resolution-2_amd/csrc tools/sg_time.cpp -o tools/_dbg/sg_time
#include "../image-super-resolution-2_amd/csrc/sgfn_tail.hip"
#include "phase_time.h"

int main() {
  const int H = 256, W = 256, c2 = 360, N = 180, HT = 12, ldh = 736;
  const long long M = (long long)H * W;
  PtRand rnd{99};
  float* h = pt_upload(rnd.f32(M * ldh));
  std::vector<float> hs(M * 2); for (size_t i = 0; i < hs.size(); i += 2) { hs[i] = 0.1f; hs[i + 1] = 1.5f; }
  float* st = pt_upload(hs);
  void* w = pt_upload(rnd.bf16((size_t)HT * 192 * 32, 0.1f));
  float* vec = pt_upload(std::vector<float>(8192, 0.05f));
  float *res = pt_zeros<float>(M * 192), *out = pt_zeros<float>(M * 192);
  auto run = [&]() { return ff_sgfn_tail(h, ldh, c2, st, vec, vec + 512, vec + 1024, vec + 5000, w, HT, vec + 6000, res, 192, out, 192, 1, H, W, N, nullptr); };
  const char* names[8] = {"start", "tables + first weight tile", "chunk 0 staged", "12 chunks done", "stores issued", "stores drained"};
  return pt_time_and_table("sgfn_tail", run, 256 * 8, 8, names);
}
