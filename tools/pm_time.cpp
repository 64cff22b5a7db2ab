// Phase timing of token_projmlp (debug aid, not part of the product): HAT geometry, 65 536 tokens x 180, hidden 360.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -DFF_TIMING -Iimage-super-resolution-2_amd/csrc tools/pm_time.cpp -o tools/_dbg/pm_time
//   tools/_dbg/pm_time [nterms = 1] [with_c2 = 1]
#include "../image-super-resolution-2_amd/csrc/token_mlp.hip"
#include "phase_time.h"

int main(int argc, char** argv) {
  const int nterms = argc > 1 ? atoi(argv[1]) : 1, with_c2 = argc > 2 ? atoi(argv[2]) : 1;
  const long long M = 65536; const int C = 180, HT = 12;
  PtRand rnd{777};
  const std::vector<float> h = rnd.f32(M * C, 2.f);
  void *dwp = pt_upload(rnd.bf16((size_t)6 * 2 * 6144, 0.15f)), *dwm = pt_upload(rnd.bf16((size_t)HT * 4 * 6144, 0.15f));
  float *att = pt_upload(h), *x = pt_upload(h), *c2 = pt_upload(h), *out = pt_zeros<float>(M * C);
  float* vec = pt_upload(std::vector<float>(4096, 0.01f));
  auto run = [&]() {
    return ff_token_projmlp(att, C, x, C, with_c2 ? c2 : nullptr, C, with_c2 ? vec : nullptr, out, C, M, C, HT, dwp, vec + 256, vec + 512, vec + 768, 1e-5f,
                            dwm, vec + 1024, vec + 2048, nterms, 0, nullptr);
  };
  const char* names[64] = {};
  names[0] = "start"; names[1] = "att gathered"; names[2] = "proj done"; names[3] = "barrier"; names[4] = "residuals added"; names[5] = "LN done";
  names[6] = "barrier"; names[40] = "MLP done"; names[41] = "stores issued"; names[42] = "stores drained";
  static char nb[64][40];
  const char* ph[4] = {"gemm1 done", "barrier", "gelu+gemm2 done", "barrier"};
  for (int ht = 0; ht < 3; ++ht) for (int k = 0; k < 4; ++k) { snprintf(nb[8 + 4 * ht + k], 40, "ht%d %s", ht, ph[k]); names[8 + 4 * ht + k] = nb[8 + 4 * ht + k]; }
  char what[64]; snprintf(what, sizeof what, "nterms %d c2 %d", nterms, with_c2);
  return pt_time_and_table(what, run, 256 * 8, 64, names);
}
