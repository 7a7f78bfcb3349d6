// Dynamic-LDS opt-in and occupancy of a kernel, for every launch site of the library.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <vector>

namespace pbbss {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per function and device, shared by all host
// threads: keep a process-wide monotonic maximum per (function, device) and only ever raise it, so
// a launch of another thread with a smaller request cannot pull it below what this one needs.
inline bool raise_lds_attribute(const void* fn, size_t lds, int dev = -1) {
  constexpr int kMaxDev = 64;
  struct Slot {
    const void* fn;
    std::atomic<size_t> have[kMaxDev];
  };
  static std::mutex mu;
  static std::vector<Slot*> slots;
  if (dev < 0) (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= kMaxDev)
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
  Slot* sl = nullptr;
  {
    std::lock_guard<std::mutex> g(mu);
    for (Slot* x : slots)
      if (x->fn == fn) sl = x;
    if (!sl) {
      sl = new Slot();
      sl->fn = fn;
      for (auto& h : sl->have) h.store(0);
      slots.push_back(sl);
    }
    if (sl->have[dev].load() >= lds) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return false;
    sl->have[dev].store(lds);
  }
  return true;
}

template <class Kfn>
inline bool raise_lds_attribute(Kfn* kfn, size_t lds) {
  return raise_lds_attribute(reinterpret_cast<const void*>(kfn), lds);
}

// Workgroups of `kfn` per compute unit at this block size and dynamic-LDS request, after the
// opt-in above; -1 on a HIP error.  The attribute and the occupancy query are host round trips
// of several microseconds each, not to be paid per launch (the GPU idles meanwhile): the answer
// is kept per thread for the last few (function, device, lds).  A hit also skips the opt-in: the
// entry was made behind one, and the attribute never falls.  The value is not clamped.
inline int blocks_per_cu(const void* kfn, int threads, size_t lds) {
  struct Entry {
    const void* fn;
    size_t lds;
    int dev, threads, occ;
  };
  constexpr int kEntries = 16;
  static thread_local Entry cache[kEntries] = {};
  static thread_local int next = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  for (const Entry& e : cache)
    if (e.fn == kfn && e.lds == lds && e.dev == dev && e.threads == threads) return e.occ;
  if (!raise_lds_attribute(kfn, lds, dev)) return -1;
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kfn, threads, lds) != hipSuccess) return -1;
  cache[next] = Entry{kfn, lds, dev, threads, occ};
  next = (next + 1) % kEntries;
  return occ;
}

template <class Kfn>
inline int blocks_per_cu(Kfn* kfn, int threads, size_t lds) {
  return blocks_per_cu(reinterpret_cast<const void*>(kfn), threads, lds);
}

}  // namespace pbbss
