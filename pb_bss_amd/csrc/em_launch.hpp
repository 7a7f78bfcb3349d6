// Host-side dispatch of the persistent EM kernel over (D, K, storage type).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "cacgmm_em.hpp"
#include "cwmm.hpp"
#include "dispatch.hpp"
#include "launch_util.hpp"

namespace pbbss {

// Split groups for the remainder bins pay a fixed price per LAUNCH (fork / join across streams
// and the members' first hand-offs, ~10 us) against ~5 us per ITERATION that an extra full
// workgroup on one compute unit costs: launches of one or two iterations -- the E- and M-steps of
// the step-wise loop -- run without them (inline aligner loop 387 -> 376 us per iteration).
constexpr int kSplitMinIterations = 3;

// launch stamp of the split protocol: never 0 (= "launcher clears the word") nor 1 (what the
// cooperative shared-weight kernel writes)
inline int next_split_epoch(const EmLaunchCfg& cfg) {
  int& e = *cfg.split_epoch;
  e = (e >= 0x7ffffff0 || e < 2) ? 2 : e + 1;
  return e;
}

constexpr int kSplitWindow = 64;      // default frames per workgroup of a split problem
constexpr int kSplitMaxProblems = 8;  // at most this many remainder problems are split

// Remainder problems as split groups.  With B = m * CUs + r (small r: the 513th bin of an
// utterance) the r extra problems would put one more full workgroup on r compute units and set
// the kernel time; each runs as G member workgroups on windows of frames instead.
struct SplitPlan {
  int window;         // frames per member workgroup (one E pass: at most 256)
  int G;              // member workgroups per problem
  int r;              // remainder problems
  size_t slab_bytes;  // exchange buffer needed: counters + error word (256 B) + slabs
  bool ok;            // the launch splits
};

// What the families decide differently (every other condition is shared).
struct SplitRule {
  int min_iterations;  // launches of fewer iterations do not pay back the fixed price (see above)
  int64_t max_B;       // larger batches hide the tail by themselves
  int64_t max_main;    // in-grid members: the B - r main problems must leave them this much room
  bool need_wt0;       // not with time-dependent weights (the members see one window each)
  bool clamped_T;      // T against two CLAMPED windows (else against two of cfg.split_window)
};
constexpr int64_t kSplitNoLimit = INT64_MAX;

// slab_doubles(r, G): exchange doubles of the family's kernel
inline SplitPlan plan_split(const EmArgs& a, const EmLaunchCfg& cfg, const SplitRule& rule,
                            size_t (*slab_doubles)(int r, int G), bool family_ok = true) {
  SplitPlan p;
  p.window = cfg.split_window > 256 ? 256 : cfg.split_window;
  p.G = (a.T + p.window - 1) / p.window;
  p.r = (int)(a.B % cfg.num_cu);
  p.slab_bytes = 256 + slab_doubles(p.r, p.G) * sizeof(double);
  p.ok = cfg.allow_split && family_ok && a.iterations >= rule.min_iterations && a.B > cfg.num_cu &&
         a.B <= rule.max_B && a.B - p.r <= rule.max_main && p.r >= 1 && p.r <= kSplitMaxProblems &&
         a.T >= 2 * (rule.clamped_T ? p.window : cfg.split_window) && (!rule.need_wt0 || a.wt == 0) &&
         p.slab_bytes <= cfg.xbuf_bytes;
  return p;
}

// exchange-buffer fields of a split launch: counters at xbuf, error word at +128, slabs at +256.
// No memsets: the arrival counters are put back to zero by the last member to leave, the error
// word is stamped with this launch's epoch (kernels without one: take_epoch = false).
inline void stamp_split(EmArgs& a, const EmLaunchCfg& cfg, const SplitPlan& p, int64_t b_first,
                        int prio, bool take_epoch = true) {
  a.T_total = a.T;
  a.split_groups = p.G;
  a.split_window = p.window;
  a.split_prio = prio;
  a.b_first = b_first;
  a.xcount = reinterpret_cast<unsigned*>(cfg.xbuf);
  a.xerror = reinterpret_cast<int*>(cfg.xbuf + 128);
  a.xslab = reinterpret_cast<double*>(cfg.xbuf + 256);
  if (take_epoch) a.xepoch = next_split_epoch(cfg);
}

// K = 1..6 and the storage type of the cACG kernels: f(K constant, float{} / double{}).
// Kernel-development builds (-DPBBSS_EM_DEV_ONLY_K=<K>) compile the one (K, float) instantiation,
// 10x faster.
template <class F>
inline int dispatch_em_k(int K, int y_is_c128, F&& f) {
#ifdef PBBSS_EM_DEV_ONLY_K
  if (y_is_c128) return PBBSS_ERR_UNSUPPORTED;
  return dispatch_list<PBBSS_EM_DEV_ONLY_K>(K, [&](auto k) { return f(k, float{}); });
#else
  return dispatch_real(y_is_c128, [&](auto y) {
    return dispatch_range<1, 6>(K, [&](auto k) { return f(k, y); });
  });
#endif
}

// The per-D entry points: each family's *_inst.hip defines the template and instantiates it for
// its -DPBBSS_EM_D, one translation unit per sensor count, so that they compile in parallel.
template <int D> int em_launch_d(int K, int y_is_c128, const EmArgs&, const EmLaunchCfg&, hipStream_t);
// packed-FP32 (reference-precision) EM kernels (em32_inst.hip); complex64 only
template <int D> int em32_launch_d(int K, const EmArgs&, const EmLaunchCfg&, hipStream_t);
// complex-Watson mixture kernels (cw_inst.hip)
template <int D> int cw_launch_d(int K, int y_is_c128, const WatsonArgs&, const EmLaunchCfg&, hipStream_t);
// joint spatial+spectral step of the cACG half (joint_inst.hip)
template <int D> int joint_launch_d(int K, int y_is_c128, const EmArgs&, const JointExtras&, int inline_pa, const EmLaunchCfg&, hipStream_t);
// spatial half of the rotated joint loop (joint_inst.hip: run_joint_ms)
template <int D> int joint_ms_launch_d(int K, int y_is_c128, const EmArgs&, const JointMs&, const EmLaunchCfg&, hipStream_t);
// EM with mixture weights shared by groups of problems (shared_inst.hip)
template <int D> int em_shared_launch_d(int K, int y_is_c128, const EmArgs&, const EmLaunchCfg&, hipStream_t);

// xxx_launch(D, ...) = xxx_launch_d<D>(...) for the compiled D = 2..8.  Not in the per-D
// translation units themselves: there the definitions are visible, and naming every D would
// instantiate all seven in each of them.
#ifndef PBBSS_EM_D
inline int em_launch(int D, int K, int y_is_c128, const EmArgs& a, const EmLaunchCfg& cfg,
                     hipStream_t s) {
  return dispatch_range<2, 8>(D, [&](auto d) { return em_launch_d<d()>(K, y_is_c128, a, cfg, s); });
}
inline int em32_launch(int D, int K, const EmArgs& a, const EmLaunchCfg& cfg, hipStream_t s) {
  return dispatch_range<2, 8>(D, [&](auto d) { return em32_launch_d<d()>(K, a, cfg, s); });
}
inline int cw_launch(int D, int K, int y_is_c128, const WatsonArgs& a, const EmLaunchCfg& cfg,
                     hipStream_t s) {
  return dispatch_range<2, 8>(D, [&](auto d) { return cw_launch_d<d()>(K, y_is_c128, a, cfg, s); });
}
inline int joint_launch(int D, int K, int y_is_c128, const EmArgs& a, const JointExtras& jx,
                        int inline_pa, const EmLaunchCfg& cfg, hipStream_t s) {
  return dispatch_range<2, 8>(
      D, [&](auto d) { return joint_launch_d<d()>(K, y_is_c128, a, jx, inline_pa, cfg, s); });
}
inline int joint_ms_launch(int D, int K, int y_is_c128, const EmArgs& a, const JointMs& jm,
                           const EmLaunchCfg& cfg, hipStream_t s) {
  return dispatch_range<2, 8>(
      D, [&](auto d) { return joint_ms_launch_d<d()>(K, y_is_c128, a, jm, cfg, s); });
}
inline int em_shared_launch(int D, int K, int y_is_c128, const EmArgs& a, const EmLaunchCfg& cfg,
                            hipStream_t s) {
  return dispatch_range<2, 8>(
      D, [&](auto d) { return em_shared_launch_d<d()>(K, y_is_c128, a, cfg, s); });
}
#endif

}  // namespace pbbss
