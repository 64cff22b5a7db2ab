// Phase timing of hab_link (debug aid, not part of the product): the HAT geometry (256x256 tokens, 16x16 windows, 6 heads of 30,
// hidden 360), wall-clock stamps per phase, averaged over waves.  Slots 0..42 are the phases of token_projmlp_bf16_kernel (the
// parent's numbers: tools/pm_time.cpp), 64 + i those of win_attn_fused_v2_kernel (tools/wf_time.cpp).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -DFF_TIMING -Iimage-super-resolution-2_amd/csrc tools/hl_time.cpp -o tools/_dbg/hl_time
//   tools/_dbg/hl_time [shift = 8]
#include "../image-super-resolution-2_amd/csrc/hab_link.hip"
#include "phase_time.h"

int main(int argc, char** argv) {
  const int shift = argc > 1 ? atoi(argv[1]) : 8;
  const int H = 256, W = 256, C = 180, LD = 192, heads = 6, d = 30, ws = 16, HT = 12;
  const long long M = (long long)H * W;
  PtRand rnd{4242};
  float* x = pt_upload(rnd.f32(M * LD, 2.f));
  const float* att = (const float*)pt_upload(rnd.bf16(M * LD, 2.f));
  const float* c2 = (const float*)pt_upload(rnd.bf16(M * LD, 2.f));
  void *dwp = pt_upload(rnd.bf16((size_t)6 * 2 * 6144, 0.15f)), *dwm = pt_upload(rnd.bf16((size_t)HT * 4 * 6144, 0.15f));
  void* wq = pt_upload(rnd.bf16((size_t)3 * heads * 2 * 32 * 192, 0.15f));
  float* rel = pt_upload(rnd.f32(heads * 31 * 48));
  float* vec = pt_upload(std::vector<float>(4096, 0.01f));
  float* qb = pt_zeros<float>(3 * heads * 32);
  float *g1 = pt_upload(std::vector<float>(192, 1.f)), *be1 = pt_zeros<float>(192);
  float* xo = pt_zeros<float>(M * LD);
  float* ao = (float*)pt_zeros<unsigned short>(M * LD);
  float* xn = (float*)pt_zeros<unsigned short>(M * LD);
  auto run = [&]() {
    return ff_hab_link(att, LD, x, LD, c2, LD, vec, 192, 1, M, xo, LD, M, C, HT, dwp, vec + 256, vec + 512, vec + 768, 1e-5f, dwm, vec + 1024, vec + 2048, 1, 3,
                       ao, LD, 0, g1, be1, 1e-5f, wq, qb, rel, 31, 48, H, W, ws, ws, shift, shift, shift > 0, heads, d, xn, LD, 1, 1, nullptr);
  };
  const char* names[128] = {};
  names[0] = "start"; names[1] = "att fragments"; names[2] = "proj done"; names[3] = "barrier"; names[4] = "residuals added"; names[5] = "LN2 done";
  names[6] = "barrier"; names[40] = "MLP done"; names[41] = "hand-over: stores issued, v built"; names[42] = "head-0 DMA + stores confirmed";
  names[66] = "LN1 done, xn stored"; names[124] = "last stores issued"; names[125] = "stores drained";
  static char nb[128][48];
  const char* ph[4] = {"gemm1 done", "gelu done", "gemm2 done", "barrier"};
  for (int ht = 0; ht < 3; ++ht) for (int k = 0; k < 4; ++k) { snprintf(nb[8 + 4 * ht + k], 48, "ht%d %s", ht, ph[k]); names[8 + 4 * ht + k] = nb[8 + 4 * ht + k]; }
  const char* ph2[8] = {"barrier W passed", "q gemm done", "k gemm+store done", "v gemm+store done", "barrier A passed", "attention done", "vmcnt(0) passed", "epilogue issued"};
  for (int hi = 0; hi < heads; ++hi) for (int k = 0; k < 8; ++k) { snprintf(nb[67 + 8 * hi + k], 48, "h%d %s", hi, ph2[k]); names[67 + 8 * hi + k] = nb[67 + 8 * hi + k]; }
  char what[64]; snprintf(what, sizeof what, "hab_link shift %d", shift);
  return pt_time_and_table(what, run, 256 * 8, 128, names);
}
