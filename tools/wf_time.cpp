// Phase timing of win_attn_fused (debug aid, not part of the product): the HAT geometry (256x256 tokens, 16x16 windows, 6 heads
// of 30), wall-clock stamps per phase, averaged over waves.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -DFF_TIMING -Iimage-super-resolution-2_amd/csrc tools/wf_time.cpp -o tools/_dbg/wf_time
//   tools/_dbg/wf_time [nterms = 1] [shift = 0] [want_xn = 1]
#include "../image-super-resolution-2_amd/csrc/win_attn_fused.hip"
#include "phase_time.h"

int main(int argc, char** argv) {
  const int nterms = argc > 1 ? atoi(argv[1]) : 1, shift = argc > 2 ? atoi(argv[2]) : 0, want_xn = argc > 3 ? atoi(argv[3]) : 1;
  const int H = 256, W = 256, C = 180, heads = 6, d = 30, ws = 16;
  const long long M = (long long)H * W;
  PtRand rnd{12345};
  float* x = pt_upload(rnd.f32(M * C, 2.f));
  float* rel = pt_upload(rnd.f32(heads * 31 * 48));
  void* w = pt_upload(rnd.bf16((size_t)3 * heads * 2 * 32 * 192, 0.15f));
  float* b = pt_zeros<float>(3 * heads * 32);
  float *g = pt_upload(std::vector<float>(192, 1.f)), *be = pt_zeros<float>(192);
  float *out = pt_zeros<float>(M * C), *xn = pt_zeros<float>(M * C);
  auto run = [&]() {
    return ff_win_attn_fused(x, C, out, C, 0, g, be, 1e-5f, w, b, rel, 31, 48, 1, H, W, H, W, ws, ws, shift, shift, shift > 0, 0, heads, d, C, 0,
                             want_xn ? xn : nullptr, C, nullptr, 0, 0, nterms, 0, 0, nullptr);
  };
  const char* names[64] = {};
  names[0] = "start"; names[1] = "tables done"; names[2] = "x gathered + LN"; names[60] = "last stores issued"; names[61] = "stores drained";
  static char nb[64][48];
  const char* ph1[8] = {"q ring passed", "q gemm done", "k ring passed", "k gemm+store done", "v gemm+store done", "barrier A passed", "attention done", "barrier B passed"};
  const char* ph2[8] = {"barrier W passed", "q gemm done", "k gemm+store done", "v gemm+store done", "barrier A passed", "attention done", "vmcnt(0) passed", "epilogue issued"};
  const char** ph = nterms == 1 ? ph2 : ph1;              // nterms 1 runs the plain-bf16 schedule (win_attn_fused_v2.inc)
  for (int hi = 0; hi < heads; ++hi) for (int k = 0; k < 8; ++k) { snprintf(nb[3 + 8 * hi + k], 48, "h%d %s", hi, ph[k]); names[3 + 8 * hi + k] = nb[3 + 8 * hi + k]; }
  char what[64]; snprintf(what, sizeof what, "nterms %d shift %d xn %d", nterms, shift, want_xn);
  return pt_time_and_table(what, run, 256 * 8, 64, names);
}
