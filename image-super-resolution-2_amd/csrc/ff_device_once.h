// "Done once per device" state of one call site: an atomic mask of the devices 0..63 already done.  No HIP in here, so the mask logic
// runs on its own under a host sanitizer (tests/device_once_tsan.cpp); ff_common.h's ff_raise_lds is its one user in the library.
#pragma once
#include <atomic>
#include <stdint.h>

struct ff_device_once {
  std::atomic<uint64_t> done{0};

  // Runs set() unless device dev is already marked, and marks it only after set() returned true.  Two threads that both see the bit clear
  // both run set(): it must be harmless to repeat.  A device index outside 0..63 has no bit: set() runs on every call.
  template <class Set>
  bool run(int dev, Set&& set) {
    const bool tracked = dev >= 0 && dev < 64;
    if (tracked && ((done.load(std::memory_order_acquire) >> dev) & 1)) return true;
    if (!set()) return false;
    if (tracked) done.fetch_or(uint64_t(1) << dev, std::memory_order_release);
    return true;
  }
};
