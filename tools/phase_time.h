// Shared by tools/*_time.cpp (debug aids, not part of the product).  Each tool includes ONE kernel source built with -DFF_TIMING
// (csrc/ff_common.h: g_ff_stamps, FF_STAMP), then this header, and keeps only its shapes, its argument set-up and its phase names.
#pragma once
#include <stdarg.h>
#include <vector>

static char g_err[512];
extern "C" const char* ff_last_error(void) { return g_err; }
void ff_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }

struct PtRand {                                         // LCG, values in [-0.5, 0.5)
  unsigned s;
  float operator()() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0f - 0.5f; }
  std::vector<float> f32(size_t n, float scale = 1.f) { std::vector<float> v(n); for (auto& x : v) x = scale * (*this)(); return v; }
  std::vector<unsigned short> bf16(size_t n, float scale) {               // truncated bf16 bit patterns
    std::vector<unsigned short> v(n);
    for (auto& x : v) { const float f = scale * (*this)(); unsigned u; memcpy(&u, &f, 4); x = (unsigned short)(u >> 16); }
    return v;
  }
};

template <class T>
static T* pt_upload(const std::vector<T>& h) {
  T* d; hipMalloc(&d, h.size() * sizeof(T)); hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice); return d;
}
template <class T>
static T* pt_zeros(size_t n) { T* d; hipMalloc(&d, n * sizeof(T)); hipMemset(d, 0, n * sizeof(T)); return d; }

// Three warm-up launches and twenty timed ones without stamps, then one launch with stamps: prints `<what>: <t> us per launch` and
// the table -- per named slot the mean / min / max time since the first wave's slot 0 over the waves that wrote it, the step of the
// mean, and the phase mean (per wave, since the previous named slot the wave wrote).  rows = blocks x 8 waves of the stamp buffer.
template <class Run>
static int pt_time_and_table(const char* what, Run run, size_t rows, int per_wave, const char* const* names) {
  g_ff_stamps = nullptr;
  for (int i = 0; i < 3; ++i) if (run()) { printf("error: %s\n", g_err); return 1; }
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipEventRecord(e0); for (int i = 0; i < 20; ++i) run(); hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  printf("%s: %.1f us per launch (no stamps)\n", what, ms * 1000 / 20);
  const size_t n = rows * per_wave;
  unsigned long long* dbg = pt_zeros<unsigned long long>(n);
  g_ff_stamps = dbg;
  if (run()) { printf("error: %s\n", g_err); return 1; }
  hipDeviceSynchronize();
  g_ff_stamps = nullptr;
  std::vector<unsigned long long> t(n);
  hipMemcpy(t.data(), dbg, n * 8, hipMemcpyDeviceToHost);
  unsigned long long t0 = ~0ull, t1 = 0;
  for (size_t i = 0; i < n; ++i) { if (i % per_wave == 0 && t[i] && t[i] < t0) t0 = t[i]; if (t[i] > t1) t1 = t[i]; }
  printf("kernel span %.2f us (first start .. last stamp), 100 MHz clock\n", (t1 - t0) / 100.0);
  double prev_mean = 0;
  std::vector<unsigned long long> last(rows, 0);        // per wave: its previous named stamp
  for (int i = 0; i < per_wave; ++i) {
    if (!names[i]) continue;
    double sum = 0, mn = 1e30, mx = 0, dsum = 0; int cnt = 0, dcnt = 0;
    for (size_t w = 0; w < rows; ++w) {
      const unsigned long long v = t[w * per_wave + i];
      if (!v) continue;
      const double u = (v - t0) / 100.0;
      sum += u; if (u < mn) mn = u; if (u > mx) mx = u; ++cnt;
      if (last[w]) { dsum += (v - last[w]) / 100.0; ++dcnt; }
      last[w] = v;
    }
    if (!cnt) continue;
    printf("%-34s mean %7.2f us (min %7.2f max %7.2f)  +%6.2f   phase mean %6.2f us   [%d waves]\n", names[i], sum / cnt, mn, mx,
           sum / cnt - prev_mean, dcnt ? dsum / dcnt : 0.0, cnt);
    prev_mean = sum / cnt;
  }
  return 0;
}
