// Phase timing of the LDS-resident 3x3 convolution (debug aid, not part of the product): HAT's CAB geometry, 256 x 256 pixels.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -DFF_TIMING -Iimage-super-resolution-2_amd/csrc tools/hx_time.cpp -o tools/_dbg/hx_time
//   tools/_dbg/hx_time <Cin> <Cout> <bn> [nterms = 1] [pool = 1]
#include "../image-super-resolution-2_amd/csrc/conv3x3_halo.hip"
#include "phase_time.h"

int main(int argc, char** argv) {
  const int Cin = argc > 1 ? atoi(argv[1]) : 60, Cout = argc > 2 ? atoi(argv[2]) : 180, bn = argc > 3 ? atoi(argv[3]) : 192;
  const int nterms = argc > 4 ? atoi(argv[4]) : 1, pool = argc > 5 ? atoi(argv[5]) : 1;
  const int H = 256, W = 256;
  const long long M = (long long)H * W;
  PtRand rnd{4242};
  float* x = pt_upload(rnd.f32(M * Cin));
  const long long wb = ff_conv3x3_halo_weight_bytes(Cout, Cin, bn, nterms);
  void* w = pt_upload(rnd.bf16(wb / 2, 0.05f));
  float *out = pt_zeros<float>(M * 192), *bias = pt_zeros<float>(256);
  const long long prow = ff_conv3x3_halo_pool_rows(1, H, W, Cout, bn, nterms);
  float* part = pt_zeros<float>(prow * bn);
  auto run = [&]() { return ff_conv3x3_halo(x, Cin, w, bn, bias, nullptr, nullptr, 0, out, Cout, 1, H, W, Cin, Cout, Cout <= 64 ? 1 : 0, 1.f, 0, (pool && Cout <= bn) ? part : nullptr, nterms, 0, nullptr); };
  const char* names[8] = {"start", "input tile staged", "taps done", "stores issued", "stores drained"};
  char what[96]; snprintf(what, sizeof what, "conv3x3 %d -> %d (bn %d, nterms %d, %lld workgroups)", Cin, Cout, bn, nterms, prow);
  return pt_time_and_table(what, run, 4096 * 8, 8, names);
}
