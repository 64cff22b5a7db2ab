// Phase timing of HAT's fused CAB (debug aid, not part of the product): 256 x 256 pixels, against the two launches it replaces.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -DFF_TIMING -Iimage-super-resolution-2_amd/csrc tools/cab_time.cpp -o tools/_dbg/cab_time
//   tools/_dbg/cab_time [B = 1]
#include "../image-super-resolution-2_amd/csrc/conv3x3_halo.hip"
#include "../image-super-resolution-2_amd/csrc/cab_fused.hip"
#include "phase_time.h"

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 1;
  const int H = 256, W = 256, Cin = 180, Cmid = 60, Cout = 180;
  const long long M = (long long)B * H * W;
  PtRand rnd{4242};
  void* xn = pt_upload(rnd.bf16(M * 192, 2.f));
  const long long wb1 = ff_conv3x3_halo_weight_bytes(Cmid, Cin, 64, 1), wb2 = ff_conv3x3_halo_weight_bytes(Cout, Cmid, 192, 1);
  void* w1 = pt_upload(rnd.bf16(wb1 / 2, 0.05f));
  void* w2 = pt_upload(rnd.bf16(wb2 / 2, 0.05f));
  float *b1 = pt_upload(rnd.f32(64, 0.5f)), *b2 = pt_upload(rnd.f32(192, 0.5f));
  unsigned short *c1 = pt_zeros<unsigned short>(M * 64), *c2 = pt_zeros<unsigned short>(M * 192), *c2p = pt_zeros<unsigned short>(M * 192);
  const long long prow = ff_conv3x3_halo_images_pool_rows(B, H, W, Cout, 192, 1);
  float *part = pt_zeros<float>(prow * 192), *partp = pt_zeros<float>(prow * 192);
  auto pair = [&]() {
    int e = ff_conv3x3_halo_images((const float*)xn, 192, w1, 64, b1, nullptr, nullptr, 0, (float*)c1, 64, B, H, W, Cin, Cmid, 1, 1.f, 0, nullptr, 1, 3, nullptr);
    return e ? e : ff_conv3x3_halo_images((const float*)c1, 64, w2, 192, b2, nullptr, nullptr, 0, (float*)c2p, 192, B, H, W, Cmid, Cout, 0, 1.f, 0, partp, 1, 3, nullptr);
  };
  auto fused = [&]() { return ff_cab_fused(xn, 192, w1, wb1, b1, w2, wb2, b2, c2, 192, part, B, H, W, Cin, Cmid, Cout, 1, 3, nullptr); };
  for (int i = 0; i < 3; ++i) if (pair()) { printf("error: %s\n", g_err); return 1; }
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipEventRecord(e0); for (int i = 0; i < 20; ++i) pair(); hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  printf("conv 180 -> 60 + GELU, conv 60 -> 180 + pool partials, two launches: %.1f us per pair\n", ms * 1000 / 20);
  const char* names[8] = {"start", "input chunk 0 staged", "conv1 taps done", "c1 tile written", "conv2 taps done", "stores issued", "stores drained"};
  char what[96]; snprintf(what, sizeof what, "cab_fused (%lld workgroups)", prow);
  const int rc = pt_time_and_table(what, fused, (size_t)prow * 8, 8, names);
  if (rc) return rc;
  // the two routes agree bit for bit (the tool's inputs, not a test: tests/test_cab_fused_gpu.py is the check)
  std::vector<unsigned short> a(M * 192), b(M * 192);
  hipMemcpy(a.data(), c2, a.size() * 2, hipMemcpyDeviceToHost); hipMemcpy(b.data(), c2p, b.size() * 2, hipMemcpyDeviceToHost);
  long long bad = 0;
  for (long long i = 0; i < M; ++i) for (int c = 0; c < Cout; ++c) bad += a[i * 192 + c] != b[i * 192 + c];
  std::vector<float> pa(prow * 192), pb(prow * 192);
  hipMemcpy(pa.data(), part, pa.size() * 4, hipMemcpyDeviceToHost); hipMemcpy(pb.data(), partp, pb.size() * 4, hipMemcpyDeviceToHost);
  long long badp = 0;
  for (size_t i = 0; i < pa.size(); ++i) badp += memcmp(&pa[i], &pb[i], 4) != 0;
  printf("c2 elements that differ from the two launches: %lld of %lld; partial sums: %lld of %zu\n", bad, M * Cout, badp, pa.size());
  return 0;
}
