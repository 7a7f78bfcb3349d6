// Joint spatial+spectral E/M step of the cACG half (gcacgmm.py / vmfcacgmm.py), one
// translation unit per sensor count D (-DPBBSS_EM_D=<D>) like em_inst.hip.
#include <cstdlib>
#include "cacgmm_em.hpp"
#include "em_launch.hpp"

#ifndef PBBSS_EM_D
#error "compile with -DPBBSS_EM_D=<sensors>"
#endif

namespace pbbss {

template <int D, int K, typename YS>
static int launch_joint(const EmArgs& a, const JointExtras& jx, int inline_pa,
                        const EmLaunchCfg& cfg, hipStream_t stream) {
  using Kern = EmKernel<D, K, YS, false>;
  size_t lds = Kern::lds_bytes(a.T) + 64;  // + class permutation of the inline PA
  // development knob: request at least this much LDS (e.g. 56000 pins two workgroups per CU)
  static const size_t lds_pad = [] {
    const char* v = getenv("PBBSS_JOINT_LDS_PAD");
    return v ? (size_t)atol(v) : (size_t)0;
  }();
  if (lds < lds_pad) lds = lds_pad;
  if (lds > cfg.lds_limit) return PBBSS_ERR_LDS_CAPACITY;
  auto kfn = inline_pa ? cacgmm_joint_kernel<D, K, YS, true>
                       : cacgmm_joint_kernel<D, K, YS, false>;
  int occ = blocks_per_cu(kfn, kEmThreads, lds);
  if (occ < 0) return PBBSS_ERR_HIP;
  if (occ < 1) occ = 1;
  // Tail handling (the rule of launch_one in em_inst.hip): with B = m * num_cu + r (small r) the
  // r extra problems would put one more full workgroup on r CUs and set the time of EVERY
  // one-iteration launch; they run as member workgroups on frame windows instead
  // (run_joint_member; no spinning, the last arriver finishes the problem).
  // The members share the grid with the main problems, at most two of which run per CU: they
  // need a third occupancy slot.  One-iteration launches split too, and the kernel takes no epoch.
  const SplitRule rule{0, 2 * (int64_t)cfg.num_cu + kSplitMaxProblems, kSplitNoLimit, false, true};
  const SplitPlan p = plan_split(
      a, cfg, rule, [](int r, int G) { return (size_t)r * G * Kern::kSlabLen; },
      !inline_pa && occ >= 3);
  if (p.ok) {  // pbbss_set_split_tail(h, 0) turns them off (A/B runs, tests)
    EmArgs ma = a;
    JointExtras mj = jx;
    ma.B = a.B - p.r;
    stamp_split(ma, cfg, p, ma.B, a.split_prio, false);
    mj.main_grid = (int)ma.B;  // <= 2 workgroups per CU: every main problem has its own block
    hipLaunchKernelGGL(kfn, dim3((unsigned)(ma.B + (int64_t)p.r * p.G)), dim3(kEmThreads), lds,
                       stream, ma, mj);
    return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
  }
  int64_t grid = (int64_t)cfg.num_cu * occ;
  if (grid > a.B) grid = a.B;
  JointExtras pj = jx;
  pj.main_grid = 0;
  hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(kEmThreads), lds, stream, a, pj);
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

// Spatial half of the rotated joint loop (run_joint_ms): one workgroup per bin, plain grid.
template <int D, int K, typename YS>
static int launch_joint_ms(const EmArgs& a, const JointMs& jm0, const EmLaunchCfg& cfg,
                           hipStream_t stream) {
  using Kern = EmKernel<D, K, YS, false>;
  size_t lds = Kern::lds_bytes(a.T);
  if (lds > cfg.lds_limit) return PBBSS_ERR_LDS_CAPACITY;
  // the helper blocks of the in-launch spectral finalize carve their totals out of the same
  // dynamic LDS
  const size_t fin_lds = (size_t)(kSpectralFinMaxW2 + 1) * sizeof(double);
  if (jm0.mode != 0 && jm0.fin.kind >= 0 && jm0.fin.helpers > 0 && lds < fin_lds) lds = fin_lds;
  JointMs jm = jm0;
  jm.lds_given = (unsigned)lds;
  auto go = [&](auto kfn) -> int {
    int occ = blocks_per_cu(kfn, kEmThreads, lds);
    if (occ < 0) return PBBSS_ERR_HIP;
    if (occ < 1) occ = 1;
    int64_t grid = (int64_t)cfg.num_cu * occ;
    if (grid > a.B) grid = a.B;
    jm.main_grid = (int)grid;
    const int helpers = (jm.mode != 0 && jm.fin.kind >= 0) ? jm.fin.helpers : 0;
    if (helpers > 0 && (lds < (size_t)(kSpectralFinMaxW2 + 1) * sizeof(double) ||
                        2 * jm.fin.K * (jm.fin.E + 1) > kSpectralFinMaxW2))
      return PBBSS_ERR_INTERNAL;  // the caller checks joint_ms_fin_supported first
    hipLaunchKernelGGL(kfn, dim3((unsigned)(grid + helpers)), dim3(kEmThreads), lds, stream, a, jm);
    return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
  };
  if (jm.mode < 0 || jm.mode > 2) return PBBSS_ERR_INVALID_ARG;
  return dispatch_range<0, 2>(
      jm.mode, [&](auto mode) { return go(cacgmm_joint_ms_kernel<D, K, YS, mode()>); });
}

template <int D>
int joint_launch_d(int K, int y_is_c128, const EmArgs& a, const JointExtras& jx, int inline_pa,
                   const EmLaunchCfg& cfg, hipStream_t stream) {
  return dispatch_em_k(K, y_is_c128, [&](auto k, auto y) {
    return launch_joint<D, k(), decltype(y)>(a, jx, inline_pa, cfg, stream);
  });
}
template int joint_launch_d<PBBSS_EM_D>(int, int, const EmArgs&, const JointExtras&, int,
                                        const EmLaunchCfg&, hipStream_t);

template <int D>
int joint_ms_launch_d(int K, int y_is_c128, const EmArgs& a, const JointMs& jm,
                      const EmLaunchCfg& cfg, hipStream_t stream) {
  return dispatch_em_k(K, y_is_c128, [&](auto k, auto y) {
    return launch_joint_ms<D, k(), decltype(y)>(a, jm, cfg, stream);
  });
}
template int joint_ms_launch_d<PBBSS_EM_D>(int, int, const EmArgs&, const JointMs&,
                                           const EmLaunchCfg&, hipStream_t);

}  // namespace pbbss
