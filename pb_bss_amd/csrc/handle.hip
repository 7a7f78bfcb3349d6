// Handle state of libpbbss_hip.so: creation and teardown, the device slabs, the process-wide
// residency gate, and the entry points that only read or set fields of the handle.  Host code only.
#include "handle.hpp"
#include <cstdio>
#include <cstdlib>
#include "comm.hpp"
#include "dhtv.hpp"

namespace pbbss {
void* Slab::grow(size_t need) {
  if (need <= bytes) return p;
  if (p) {
    if (hipDeviceSynchronize() != hipSuccess) return nullptr;
    release();
  }
  if (hipMalloc(&p, need) != hipSuccess) {
    p = nullptr;
    return nullptr;
  }
  bytes = need;
  return p;
}

void Slab::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  bytes = 0;
}

ResidencyGate::State& ResidencyGate::state(int dev) {
  static State st[kMaxDev];
  return st[dev < 0 || dev >= kMaxDev ? 0 : dev];
}

bool ResidencyGate::enabled() {
  static const bool on = [] {
    const char* v = getenv("PBBSS_RESIDENCY_GATE");
    return !(v && v[0] == '0');
  }();
  return on;
}

ResidencyGate::ResidencyGate(pbbss_handle_t h_, hipStream_t s_, bool needed)
    : h(h_), s(s_), active(false) {
  if (!needed || !h || h->gate_dev < 0 || !enabled()) return;
  State& st = state(h->gate_dev);
  st.mu.lock();
  if (st.handles < 2) {  // nobody to collide with
    st.mu.unlock();
    return;
  }
  // The device mutex stays held until the destructor has recorded this launch's completion
  // event: the host-side ENQUEUE of gated launches is serialised (the device work is not waited
  // for), so a second thread always finds the event of the launch in front of it.  The lock
  // spans the entry point's body: normally microseconds, but a body that has to GROW one of the
  // handle's slabs (Slab::grow: hipDeviceSynchronize + hipFree + hipMalloc, first call at a
  // larger shape only) does so under the lock, and other threads' gated calls wait behind it
  // once.
  // (Until round 5 the lock was dropped in between: two threads entering together both waited
  // for the same older event and then ran side by side -- the residual "not co-resident" case
  // of tests/test_gpu_contention.py, about one full-suite run in ten.)
  active = true;
  if (st.last && !(st.owner == h && st.owner_stream == s)) (void)hipStreamWaitEvent(s, st.last, 0);
}

ResidencyGate::~ResidencyGate() {
  if (!active) return;
  State& st = state(h->gate_dev);
  if (hipEventRecord(h->gate_ev, s) == hipSuccess) {
    st.last = h->gate_ev;
    st.owner = h;
    st.owner_stream = s;
  }
  st.mu.unlock();
}

void ResidencyGate::on_create(pbbss_handle_t h, int dev) {
  if (dev < 0 || dev >= kMaxDev) return;
  if (hipEventCreateWithFlags(&h->gate_ev, hipEventDisableTiming) != hipSuccess) {
    h->gate_ev = nullptr;
    return;
  }
  h->gate_dev = dev;
  State& st = state(dev);
  // the gate becomes active with the second handle: whatever the first one has in flight was
  // launched without leaving an event behind -- let it drain once (outside the lock: a gated
  // launch of another thread must not wait behind a device-wide synchronisation)
  bool drain;
  {
    std::lock_guard<std::recursive_mutex> g(st.mu);
    drain = ++st.handles == 2;
  }
  if (drain) (void)hipDeviceSynchronize();
}

void ResidencyGate::on_destroy(pbbss_handle_t h) {
  if (h->gate_dev < 0) return;  // never registered
  State& st = state(h->gate_dev);
  {
    std::lock_guard<std::recursive_mutex> g(st.mu);
    --st.handles;
    if (st.owner == h) {
      st.last = nullptr;
      st.owner = nullptr;
      st.owner_stream = nullptr;
    }
  }
  if (h->gate_ev) (void)hipEventDestroy(h->gate_ev);
}
}  // namespace pbbss

using pbbss::DeviceGuard, pbbss::ResidencyGate;

namespace {
// The split-bin groups must run CONCURRENTLY with the main EM launch.  HIP maps streams onto
// a handful of hardware queues round-robin; a plain extra stream can land on the queue of the
// caller's stream (observed after RCCL had created its own streams: the two launches then
// serialise, 1.7 -> 2.4 ms).  A stream of a different (highest) priority lives on a separate
// set of queues.
bool make_side_stream(hipStream_t* out) {
  const bool dbg = getenv("PBBSS_DEBUG") != nullptr;
  int least = 0, greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (dbg) fprintf(stderr, "pbbss: priority range rc=%d least=%d greatest=%d\n", (int)e, least, greatest);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    greatest = 0;
  }
  e = hipStreamCreateWithPriority(out, hipStreamNonBlocking, greatest);
  if (dbg) fprintf(stderr, "pbbss: hipStreamCreateWithPriority rc=%d (%s)\n", (int)e, hipGetErrorString(e));
  if (e == hipSuccess) return true;
  (void)hipGetLastError();
  e = hipStreamCreateWithFlags(out, hipStreamNonBlocking);
  if (dbg) fprintf(stderr, "pbbss: hipStreamCreateWithFlags rc=%d (%s)\n", (int)e, hipGetErrorString(e));
  return e == hipSuccess;
}

void* handle_scratch(void* ctx, size_t bytes) {
  return static_cast<pbbss_handle_t>(ctx)->scratch.grow(bytes);
}

// Everything the handle owns on the device, in the order pbbss_create relies on.  The handle's
// device is current.
int create_device_state(pbbss_handle_t h) {
  h->cfg.xbuf_bytes = (size_t)1 << 20;
  void* xb = nullptr;
  if (hipMalloc(&xb, h->cfg.xbuf_bytes) != hipSuccess) return PBBSS_ERR_HIP;
  h->cfg.xbuf = static_cast<char*>(xb);
  if (!make_side_stream(&h->cfg.side_stream) ||
      hipEventCreateWithFlags(&h->cfg.ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->cfg.ev_join, hipEventDisableTiming) != hipSuccess)
    return PBBSS_ERR_HIP;
  // arrival counters / error words start at zero (the joint launch's members reset their
  // counter themselves; the EM split launch clears its own before every launch)
  if (hipMemset(xb, 0, 256) != hipSuccess) return PBBSS_ERR_HIP;
  h->team_bytes = (size_t)4 << 20;
  if (hipMalloc(&h->team_buf, h->team_bytes) != hipSuccess) {
    h->team_buf = nullptr;  // the one-workgroup kernel needs none
    h->team_bytes = 0;
  }
  for (int i = 0; i < pbbss_handle_s::kTimingRing; ++i) {
    if (hipEventCreate(&h->ring0[i]) != hipSuccess || hipEventCreate(&h->ring1[i]) != hipSuccess)
      return PBBSS_ERR_HIP;
  }
  ResidencyGate::on_create(h, h->device);
  return PBBSS_OK;
}

// The one teardown: of a complete handle (pbbss_destroy) and of whatever part of one
// create_device_state got to before a runtime call failed.
void destroy_handle(pbbss_handle_t h) {
  for (int i = 0; i < pbbss_handle_s::kTimingRing; ++i) {
    if (h->ring0[i]) (void)hipEventDestroy(h->ring0[i]);
    if (h->ring1[i]) (void)hipEventDestroy(h->ring1[i]);
  }
  h->scratch.release();
  h->work.release();
  if (h->comm) (void)pbbss::comm_destroy(h->comm);
  h->comm_buf.release();
  if (h->team_buf) (void)hipFree(h->team_buf);
  if (h->cfg.xbuf) (void)hipFree(h->cfg.xbuf);
  if (h->cfg.side_stream) (void)hipStreamDestroy(h->cfg.side_stream);
  if (h->cfg.ev_fork) (void)hipEventDestroy(h->cfg.ev_fork);
  if (h->cfg.ev_join) (void)hipEventDestroy(h->cfg.ev_join);
  ResidencyGate::on_destroy(h);
  delete h;
}
}  // namespace

PBBSS_API int pbbss_version(void) { return PBBSS_VERSION; }

PBBSS_API const char* pbbss_error_string(int code) {
  switch (code) {
    case PBBSS_OK: return "ok";
    case PBBSS_ERR_INVALID_ARG: return "invalid argument";
    case PBBSS_ERR_UNSUPPORTED:
      return "shape not covered by the compiled kernels (2 <= D <= 32 sensors, 8 for LCMV; the "
             "class range of every entry point is stated in pbbss.h)";
    case PBBSS_ERR_HIP: return "HIP runtime error";
    case PBBSS_ERR_LDS_CAPACITY:
      return "observation does not fit the LDS-resident EM kernel (too many frames)";
    case PBBSS_ERR_INTERNAL: return "workspace accounting mismatch inside the library (a bug)";
    default: return "unknown error";
  }
}

PBBSS_API int pbbss_create(pbbss_handle_t* out, int device_id) {
  if (!out) return PBBSS_ERR_INVALID_ARG;
  const bool dbg = getenv("PBBSS_DEBUG") != nullptr;
  // bind to device_id for the allocations below, then give the caller its current device back
  // (every other entry point uses DeviceGuard; a lazily created handle must not move the
  // process's current device)
  int prev_device = -1;
  (void)hipGetDevice(&prev_device);
  struct Restore {
    int dev;
    ~Restore() {
      if (dev >= 0) (void)hipSetDevice(dev);
    }
  } restore{prev_device};
  hipError_t e0 = hipSetDevice(device_id);
  if (dbg) fprintf(stderr, "pbbss: hipSetDevice(%d) rc=%d (%s)\n", device_id, (int)e0, hipGetErrorString(e0));
  if (e0 != hipSuccess) return PBBSS_ERR_HIP;
  hipDeviceProp_t prop;
  e0 = hipGetDeviceProperties(&prop, device_id);
  if (dbg) fprintf(stderr, "pbbss: hipGetDeviceProperties rc=%d (%s)\n", (int)e0, hipGetErrorString(e0));
  if (e0 != hipSuccess) return PBBSS_ERR_HIP;
  pbbss_handle_t h = new pbbss_handle_s();
  h->device = device_id;
  h->cfg.num_cu = prop.multiProcessorCount;
  // gfx950: 160 KiB per CU, one workgroup may take all of it
  size_t lds = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor
                                                     : prop.sharedMemPerBlock;
  if (lds < prop.sharedMemPerBlock) lds = prop.sharedMemPerBlock;
  h->cfg.lds_limit = lds;
  h->cfg.get_scratch = handle_scratch;
  h->cfg.scratch_ctx = h;
  h->cfg.allow_split = 1;
  h->cfg.split_window = pbbss::kSplitWindow;
  // wave priority of the remainder bin's member workgroups (s_setprio): 1, above the full
  // workgroups.  At priority 0 the MAIN kernel gets faster (1.43 -> 1.37 ms; with the full
  // workgroups raised to 1 even 1.26 ms, the 512-bin time) but the members then only harvest idle
  // issue slots and need 1.72 ms for their 100 iterations: the step waits for them
  // (profiles/r03_g_member_priority.txt).  The packed-FP32 kernel's members sit in the same grid,
  // where the kernel time shows it directly: 1.05 ms at 1, 1.29 ms at 0.
  h->cfg.split_prio = 1;
  h->cfg.split_prio32 = 1;
  if (const char* p = getenv("PBBSS_SPLIT_PRIO")) h->cfg.split_prio = h->cfg.split_prio32 = atoi(p);
  h->cfg.split_epoch = &h->split_epoch;
  if (const char* w = getenv("PBBSS_SPLIT_WINDOW")) {
    int v = atoi(w);
    if (v >= 64 && v % 64 == 0) h->cfg.split_window = v;
  }
  if (const char* tv = getenv("PBBSS_DHTV_TEAM")) h->dhtv_team = atoi(tv);
  const int rc = create_device_state(h);
  if (rc != PBBSS_OK) {
    destroy_handle(h);
    return rc;
  }
  *out = h;
  return PBBSS_OK;
}

PBBSS_API int pbbss_destroy(pbbss_handle_t h) {
  if (!h) return PBBSS_ERR_INVALID_ARG;
  destroy_handle(h);
  return PBBSS_OK;
}

PBBSS_API int pbbss_set_timing(pbbss_handle_t h, int enable) {
  if (!h) return PBBSS_ERR_INVALID_ARG;
  h->timing = enable ? 1 : 0;
  return PBBSS_OK;
}

PBBSS_API int pbbss_set_phase_profile(pbbss_handle_t h, void* dev_counters) {
  if (!h) return PBBSS_ERR_INVALID_ARG;
  h->prof = static_cast<unsigned long long*>(dev_counters);
  return PBBSS_OK;
}

PBBSS_API int pbbss_set_split_tail(pbbss_handle_t h, int enable) {
  if (!h) return PBBSS_ERR_INVALID_ARG;
  h->cfg.allow_split = enable ? 1 : 0;
  return PBBSS_OK;
}

PBBSS_API int pbbss_set_dhtv_team(pbbss_handle_t h, int workgroups_per_utterance) {
  if (!h || workgroups_per_utterance < -pbbss::kDhtvTeamMax || workgroups_per_utterance > 64 ||
      workgroups_per_utterance == -1)
    return PBBSS_ERR_INVALID_ARG;
  h->dhtv_team = workgroups_per_utterance;
  return PBBSS_OK;
}

PBBSS_API int pbbss_set_dhtv_probe(pbbss_handle_t h, int enable) {
  if (!h) return PBBSS_ERR_INVALID_ARG;
  if (enable < 0 || enable > 3) return PBBSS_ERR_INVALID_ARG;
  h->dhtv_probe = enable;
  return PBBSS_OK;
}

PBBSS_API int pbbss_set_spin_limit(pbbss_handle_t h, unsigned polls) {
  DeviceGuard device_guard(h);
  if (!h) return PBBSS_ERR_INVALID_ARG;
  h->cfg.spin_limit = polls;
  return PBBSS_OK;  // (the DHTV team kernels take it as a kernel argument since round 6)
}

PBBSS_API int pbbss_split_error(pbbss_handle_t h, int* out_flag) {
  DeviceGuard device_guard(h);
  if (!h || !out_flag) return PBBSS_ERR_INVALID_ARG;
  int v = 0;
  if (hipMemcpy(&v, h->cfg.xbuf + 192, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return PBBSS_ERR_HIP;
  *out_flag = v;
  return PBBSS_OK;
}

PBBSS_API int pbbss_split_reset(pbbss_handle_t h) {
  DeviceGuard device_guard(h);
  if (!h || !h->cfg.xbuf) return PBBSS_ERR_INVALID_ARG;
  // every launch of this handle must have left the device: a member still running would see its
  // arrival counter vanish.  Then the counters, the per-launch error word and the sticky flag of
  // pbbss_split_error go back to their creation state (a launch that was aborted half-way -- a
  // device fault, a debug-build trap, a timed-out hand-off -- leaves the counters non-zero, and
  // every later split launch of the handle would pass its barriers early or time out).
  if (hipDeviceSynchronize() != hipSuccess) return PBBSS_ERR_HIP;
  if (hipMemset(h->cfg.xbuf, 0, 256) != hipSuccess) return PBBSS_ERR_HIP;
  return PBBSS_OK;
}

PBBSS_API int pbbss_kernel_ms_lagged(pbbss_handle_t h, int lag, float* out_ms) {
  DeviceGuard device_guard(h);
  if (!h || !out_ms) return PBBSS_ERR_INVALID_ARG;
  if (!h->timing) return PBBSS_ERR_INVALID_ARG;
  if (lag < 0 || lag >= pbbss_handle_s::kTimingRing || (unsigned)lag >= h->ring_seq)
    return PBBSS_ERR_INVALID_ARG;
  const int slot = (int)((h->ring_seq - 1 - (unsigned)lag) % pbbss_handle_s::kTimingRing);
  if (hipEventSynchronize(h->ring1[slot]) != hipSuccess) return PBBSS_ERR_HIP;
  if (hipEventElapsedTime(&h->last_ms, h->ring0[slot], h->ring1[slot]) != hipSuccess)
    return PBBSS_ERR_HIP;
  *out_ms = h->last_ms;
  return PBBSS_OK;
}

PBBSS_API int pbbss_last_kernel_ms(pbbss_handle_t h, float* out_ms) {
  return pbbss_kernel_ms_lagged(h, 0, out_ms);
}
