// The library handle (pbbss_handle_t) and the host-side helpers every entry point of the C-ABI
// layer uses: device slabs and their carver, device / timing / residency guards.  Host code only.
#pragma once
#include "pbbss.h"
#include <mutex>
#include "carver.hpp"
#include "embed.hpp"
#include "embed_wide.hpp"
#include "em_launch.hpp"

#define PBBSS_API extern "C" __attribute__((visibility("default")))

namespace pbbss {
// Grow-only device slab.  Growing synchronises the device (hipDeviceSynchronize before the free)
// -- it happens at most a few times per process, at the first call of a larger shape; a request
// the slab already covers touches the runtime not at all.
struct Slab {
  void* p = nullptr;
  size_t bytes = 0;
  void* grow(size_t need);  // the slab, at least `need` bytes long; null if the runtime refused
  void release();
};
}  // namespace pbbss

struct pbbss_handle_s {
  int device = 0;
  pbbss::EmLaunchCfg cfg{};
  pbbss::Slab scratch;   // frame arrays of utterances too long for LDS (cfg.get_scratch)
  pbbss::Slab work;      // workspaces of the multi-kernel mixture loops
  void* comm = nullptr;  // RCCL communicator of pbbss_comm_create (one rank = this process), or null
  int comm_world = 1, comm_rank = 0;
  int split_epoch = 1;   // launch stamp of the split protocol (em_inst.hip: next_split_epoch)
  // pack / gather buffers of pbbss_allgather_masks: owned by the communicator, never shared with
  // the work slab (a collective may still be in flight)
  pbbss::Slab comm_buf;
  void* team_buf = nullptr;  // control words + centroid partials of the DHTV team kernel
  size_t team_bytes = 0;
  int dhtv_team = 0;   // workgroups per utterance (0 = default, 1 = one-workgroup kernel)
  int dhtv_probe = 0;  // all-segments-at-once identity probe in front of the plan (pbbss_set_dhtv_probe)
  unsigned long long* prof = nullptr;
  int timing = 0;
  float last_ms = 0.f;
  // timed regions record into a ring of event pairs, so that a caller can read the duration of an
  // OLDER launch without draining the queue (pbbss_kernel_ms_lagged)
  static constexpr int kTimingRing = 4;
  hipEvent_t ring0[kTimingRing] = {}, ring1[kTimingRing] = {};
  unsigned ring_seq = 0;         // timed regions started so far
  hipEvent_t gate_ev = nullptr;  // completion of this handle's last launch with inter-workgroup waits
  int gate_dev = -1;  // device index of the residency gate this handle takes part in (-1: none)
  float bss_phase_ms[4] = {};  // phases of the last timed pbbss_bss_eval (pbbss_bss_eval_phase_ms)
};

namespace pbbss {
inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// standalone embedding entry points: K <= kEmbedMaxK on the kernels of embed.hip, beyond on the
// class tiles of embed_wide.hip
inline bool embed_shape_ok(int64_t B, int64_t N, int E, int K) {
  return B >= 1 && B <= 65535 && N >= 1 && E >= 1 && E <= kEmbedMaxE && K >= 1 &&
         K <= kEmbedWideMaxK;
}

// Carve a workspace out of `slab`.  `pieces(Carver&)` lists the take() calls ONCE; it runs on a
// measuring carver, the slab grows to that count, and it runs again on the slab -- so the bytes
// asked for cannot disagree with the pointers handed out.
template <typename Pieces>
int carve(Slab& slab, Pieces&& pieces) {
  Carver measure;
  pieces(measure);
  void* p = slab.grow(measure.off);
  if (!p) return PBBSS_ERR_HIP;
  Carver wc(p);
  pieces(wc);
  return PBBSS_OK;
}

// Every entry point runs with the handle's device current (a caller holding tensors on several
// GPUs in one process may have another one selected) and restores the caller's selection.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(pbbss_handle_t h) {
    if (!h) return;
    if (hipGetDevice(&prev) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    if (prev != h->device) switched = (hipSetDevice(h->device) == hipSuccess);
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

struct TimedRegion {
  pbbss_handle_t h;
  hipStream_t s;
  int slot = 0;
  TimedRegion(pbbss_handle_t h_, hipStream_t s_) : h(h_), s(s_) {
    if (h->timing) {
      slot = (int)(h->ring_seq++ % pbbss_handle_s::kTimingRing);
      (void)hipEventRecord(h->ring0[slot], s);
    }
  }
  ~TimedRegion() {
    if (h->timing) (void)hipEventRecord(h->ring1[slot], s);
  }
};

// ---------------------------------------------------------------------------------------------
// Residency gate (round 4).  Kernels whose workgroups WAIT for each other -- split groups of a
// remainder bin, the cooperative shared-weight kernel, in-grid members, DHTV teams -- need their
// peers on the chip at the same time.  Two such kernels launched concurrently from two handles
// (host threads / streams) of one process can starve each other: each holds compute-unit slots
// while it waits for peers that only fit once the other one lets go (round 3 measured the
// cooperative kernel "not served" in 2-16 % of the fits that ran beside a packed-FP32 fit,
// profiles/r03_i_coop_contention_probe.txt; the bounded waits turn the stall into a repeat, never
// a hang).  The gate removes the situation instead of riding it out: per device, every launch of
// that kind first waits (stream-ordered, hipStreamWaitEvent) for the completion event of the
// previous one -- whichever handle issued it -- and leaves its own completion event behind.  With
// a single handle on the device the gate does nothing at all (stream order already serialises its
// launches); PBBSS_RESIDENCY_GATE=0 switches it off.  The entry points arm it only for calls that
// CAN launch such a kernel (`needed`: may_split() for the fused fits, always for the cooperative
// shared-weight fit and the DHTV solver): plain fits -- no remainder bin, fewer than three
// iterations, generic-size path, the joint models (their members never wait) -- keep their
// multi-stream concurrency beside other handles.  Within one process the gate orders the GATED
// launches exactly since round 5 (their enqueue is serialised, see the constructor).  It does
// not order ungated work: a plain fit, a joint fit or a generic-size fit of another handle can
// still hold compute units while a gated kernel's members are being placed -- for that case,
// and for work of OTHER processes on the device, the bounded waits and the host-side repeats
// remain the safety net.
// The state table is process-wide: state(), enabled() and everything that touches the table are
// defined once, in handle.hip, so that every translation unit that arms a gate shares it.
struct ResidencyGate {
  static constexpr int kMaxDev = 64;
  struct State {
    std::recursive_mutex mu;  // recursive: a gated entry point may create / destroy a handle
    hipEvent_t last = nullptr;        // completion of the most recent gated launch on this device
    pbbss_handle_t owner = nullptr;   // handle whose gate_ev `last` is
    hipStream_t owner_stream = nullptr;
    int handles = 0;                  // live handles on this device
  };
  static State& state(int dev);
  static bool enabled();
  pbbss_handle_t h;
  hipStream_t s;
  bool active;
  ResidencyGate(pbbss_handle_t h_, hipStream_t s_, bool needed = true);
  ~ResidencyGate();
  static void on_create(pbbss_handle_t h, int dev);
  static void on_destroy(pbbss_handle_t h);
  // Can a fused fit of B problems launch workgroups that wait for each other (split groups /
  // in-grid members of the remainder problems: em_inst.hip, em32_inst.hip, cw_inst.hip)?  A
  // superset of the launchers' own conditions, from the arguments alone.
  static bool may_split(pbbss_handle_t h, int64_t B, int D, int iterations) {
    if (!h) return false;
    const int64_t cu = h->cfg.num_cu > 0 ? h->cfg.num_cu : 256;
    return D <= 8 && iterations >= kSplitMinIterations && B > cu && B % cu != 0;
  }
};
}  // namespace pbbss
