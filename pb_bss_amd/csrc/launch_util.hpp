// What every launch site of the library shares: the launch configuration of the handle
// (EmLaunchCfg) with its side-stream fork / join, dynamic-LDS opt-in and occupancy of a kernel,
// and the device-to-device copies of the fits.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include "pbbss.h"
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

inline int copy_d2d(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (dst == src || bytes == 0) return PBBSS_OK;
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess ? PBBSS_OK
                                                                                   : PBBSS_ERR_HIP;
}

// "model in -> model out" of a fit that starts from a model: the loops keep the model in the
// caller's output arrays.  One array of a model: mean / scale or covariance / weight of the
// embedding mixtures, eigvec / eigval / weight or mode / concentration / weight of the spatial ones.
struct ModelPart {
  void* dst;
  const void* src;
  size_t bytes;
};
inline int copy_model(const ModelPart& a, const ModelPart& b, const ModelPart& c, hipStream_t s) {
  for (const ModelPart* p : {&a, &b, &c}) {
    const int rc = copy_d2d(p->dst, p->src, p->bytes, s);
    if (rc != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}


struct EmLaunchCfg {
  int num_cu;        // compute units of the bound device
  size_t lds_limit;  // usable LDS bytes per workgroup
  // grow-only device scratch owned by the handle (frame arrays of long utterances)
  void* (*get_scratch)(void* ctx, size_t bytes);
  void* scratch_ctx;
  // split-bin remainder launches: side stream + fork/join events + exchange buffer
  hipStream_t side_stream;
  hipEvent_t ev_fork, ev_join;
  char* xbuf;        // [xbuf_bytes] device memory: counters, error word, slabs
  size_t xbuf_bytes;
  int allow_split;   // 0 disables the split variant (tests / debugging)
  int split_window;  // frames per workgroup of a split problem (multiple of 64)
  int split_prio;    // s_setprio level of the split waves (float64 kernels)
  int split_prio32;  // ... of the packed-FP32 kernel's member workgroups
  int* split_epoch;  // host counter stamping the launches of the split protocol
  unsigned spin_limit;  // EmArgs::spin_limit of every launch (0: the kernels' defaults)
  // kernel timing (pbbss_set_timing): start / stop events attached to the DISPATCH of the EM kernel
  // itself (hipExtLaunchKernelGGL: timestamps of the kernel's own completion signal) instead of
  // two hipEventRecord packets around the call -- those cost ~30 us of queue time per step
  // (tools/launch_gap.py).  Null: timing off.
  hipEvent_t ev_t0, ev_t1;
};

// ---- the handle's side stream: work that runs beside the caller's stream ------------------------
// side_fork: everything enqueued on `stream` so far precedes what goes onto cfg.side_stream next.
// side_join: `stream` waits for everything enqueued on cfg.side_stream so far.
// One error policy for every user: once anything may have been enqueued on the side stream the
// join is always issued -- the caller's stream must cover all that was enqueued -- and the first
// error is returned.  An error before that point returns at once: there is nothing to join.
inline int side_fork_record(const EmLaunchCfg& cfg, hipStream_t stream) {
  return hipEventRecord(cfg.ev_fork, stream) == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}
inline int side_fork_wait(const EmLaunchCfg& cfg) {
  return hipStreamWaitEvent(cfg.side_stream, cfg.ev_fork, 0) == hipSuccess ? PBBSS_OK
                                                                           : PBBSS_ERR_HIP;
}
inline int side_fork(const EmLaunchCfg& cfg, hipStream_t stream) {
  const int rc = side_fork_record(cfg, stream);
  return rc != PBBSS_OK ? rc : side_fork_wait(cfg);
}
inline int side_join_record(const EmLaunchCfg& cfg) {
  return hipEventRecord(cfg.ev_join, cfg.side_stream) == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}
inline int side_join_wait(const EmLaunchCfg& cfg, hipStream_t stream) {
  return hipStreamWaitEvent(stream, cfg.ev_join, 0) == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}
inline int side_join(const EmLaunchCfg& cfg, hipStream_t stream) {
  const int rc = side_join_record(cfg);
  return rc != PBBSS_OK ? rc : side_join_wait(cfg, stream);
}

// main() on `stream` and side(cfg.side_stream) beside it.  The fork point is recorded first, but
// main() is enqueued BEFORE the side stream is touched: preparing the side stream (fork wait,
// launch, join record) is a handful of host calls during which the device would otherwise idle,
// and what runs there is independent of main's work and finishes long before it.  A failed main()
// returns before the side stream has seen anything; after that the join is always issued.
template <class Main, class Side>
inline int with_side_stream(const EmLaunchCfg& cfg, hipStream_t stream, Main&& main, Side&& side) {
  int rc;
  if ((rc = side_fork_record(cfg, stream)) != PBBSS_OK) return rc;
  if ((rc = main()) != PBBSS_OK) return rc;
  if ((rc = side_fork_wait(cfg)) != PBBSS_OK) return rc;
  rc = side(cfg.side_stream);
  const int rc_join = side_join(cfg, stream);
  return rc != PBBSS_OK ? rc : rc_join;
}

}  // namespace pbbss
