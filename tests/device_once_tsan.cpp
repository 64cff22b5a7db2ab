// Host-only check of csrc/ff_device_once.h, the once-per-device mask behind ff_raise_lds: 8 threads, devices 0, 1, 63 and 64, no HIP.
//   c++ -std=c++17 -O1 -g -pthread -fsanitize=thread -I image-super-resolution-2_amd/csrc tests/device_once_tsan.cpp -o /tmp/device_once_tsan && /tmp/device_once_tsan
// (tests/test_device_once_cpu.py builds and runs it without the sanitizer.)  Checked for every device with a bit (0, 1, 63):
//   - a caller either saw the bit set, or ran the setter and then published: the setter ran at least once and at most once per thread
//     that can have seen the bit clear, and never again once every thread has met at the barrier;
//   - what the setter wrote (the stand-in for the attribute: a relaxed atomic, since two first callers may both set it, as they may
//     both call hipFuncSetAttribute) is visible to a caller that skipped the setter: the release / acquire pair on the mask;
//   - a failing setter publishes nothing: the next call runs it again.
// Device 64 has no bit: the setter runs on every call.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "ff_device_once.h"

static std::atomic<int> fails{0};
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++fails; } \
  } while (0)

int main() {
  constexpr int NT = 8, ROUNDS = 200, CALLS = 50;
  const int devs[4] = {0, 1, 63, 64};

  {  // a failing setter leaves the bit clear
    ff_device_once once;
    int runs = 0;
    CHECK(!once.run(5, [&] { ++runs; return false; }));
    CHECK(once.done.load() == 0);
    CHECK(once.run(5, [&] { ++runs; return true; }));
    CHECK(once.run(5, [&] { ++runs; return true; }));
    CHECK(runs == 2 && once.done.load() == (uint64_t(1) << 5));
    CHECK(once.run(-1, [&] { ++runs; return true; }) && once.run(64, [&] { ++runs; return true; }) && runs == 4);
    CHECK(once.done.load() == (uint64_t(1) << 5));
  }

  for (int round = 0; round < ROUNDS; ++round) {
    ff_device_once once;
    std::atomic<int> attr[4], set_runs[4], skipped[4], go{0};   // attr: relaxed, so a reader relies on the mask's ordering alone
    for (int d = 0; d < 4; ++d) { attr[d] = 0; set_runs[d] = 0; skipped[d] = 0; }
    std::vector<std::thread> th;
    for (int t = 0; t < NT; ++t)
      th.emplace_back([&, t] {
        go.fetch_add(1);
        while (go.load() < NT) { }                    // all threads make their first call together
        for (int c = 0; c < CALLS; ++c)
          for (int k = 0; k < 4; ++k) {
            const int d = (k + t) & 3;
            bool ran = false;
            const bool ok = once.run(devs[d], [&] {
              attr[d].store(1, std::memory_order_relaxed);
              set_runs[d].fetch_add(1);
              ran = true;
              return true;
            });
            if (!ok) { ++fails; return; }
            if (!ran) {
              skipped[d].fetch_add(1);
              if (attr[d].load(std::memory_order_relaxed) != 1) ++fails;   // skipped the setter: its write must be visible
            }
          }
      });
    for (auto& x : th) x.join();
    for (int d = 0; d < 3; ++d) {
      CHECK(set_runs[d] >= 1 && set_runs[d] <= NT);
      CHECK(set_runs[d] + skipped[d] == NT * CALLS);
      CHECK((once.done.load() >> devs[d]) & 1);
    }
    CHECK(set_runs[3] == NT * CALLS && skipped[3] == 0);
    CHECK(once.done.load() == ((uint64_t(1) << 0) | (uint64_t(1) << 1) | (uint64_t(1) << 63)));
    int late = 0;                                     // after the join nobody runs a setter for a device with a bit
    for (int d = 0; d < 3; ++d) once.run(devs[d], [&] { ++late; return true; });
    CHECK(late == 0);
  }
  if (fails) printf("device_once: %d checks FAILED\n", fails.load());
  else printf("device_once: ok (8 threads, devices 0 1 63 64)\n");
  return fails ? 1 : 0;
}
