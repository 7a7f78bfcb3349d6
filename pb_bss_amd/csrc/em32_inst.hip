// Packed-FP32 (reference-precision) EM kernel: one translation unit per sensor count D
// (compiled with -DPBBSS_EM_D=<D>), as em_inst.hip.
#include "cacgmm_em32.hpp"
#include "em_launch.hpp"

#ifndef PBBSS_EM_D
#error "compile with -DPBBSS_EM_D=<sensors>"
#endif

namespace pbbss {

template <int D, int K>
static int launch32(EmArgs a, const EmLaunchCfg& cfg, hipStream_t stream) {
  using Kern = EmKernel32<D, K>;
  const size_t lds = Kern::lds_bytes(a.T);
  if (lds > cfg.lds_limit) return PBBSS_ERR_LDS_CAPACITY;  // no HBM-scratch variant of this kernel
  auto kfn = cacgmm_em32_kernel<D, K>;
  int occ = blocks_per_cu(kfn, kEmThreads, lds);
  if (occ < 0) return PBBSS_ERR_HIP;
  if (occ < 1) occ = 1;
  // Remainder problems as split groups (em_launch.hpp), here in the SAME grid behind the full
  // workgroups -- they need a free occupancy slot next to them.
  const SplitRule rule{kSplitMinIterations, kSplitNoLimit, (int64_t)cfg.num_cu * (occ - 1), false,
                       false};
  const SplitPlan p = plan_split(a, cfg, rule, Kern::Base::split_slab_doubles);
  int64_t grid = (int64_t)cfg.num_cu * occ;
  if (p.ok) {
    a.B -= p.r;
    if (grid > a.B) grid = a.B;
    a.main_grid = (int)grid;
    grid += (int64_t)p.r * p.G;
    stamp_split(a, cfg, p, a.B, cfg.split_prio32);
  } else if (grid > a.B) {
    grid = a.B;
  }
  a.lds_given = (unsigned)lds;
  if (a.xcount) a.xbuf_given = (unsigned)cfg.xbuf_bytes;
  if (cfg.ev_t0) {
    hipExtLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(kEmThreads), lds, stream, cfg.ev_t0,
                          cfg.ev_t1, 0, a);
  } else {
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(kEmThreads), lds, stream, a);
  }
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

template <int D>
int em32_launch_d(int K, const EmArgs& a, const EmLaunchCfg& cfg, hipStream_t stream) {
  return dispatch_range<1, 6>(K, [&](auto k) { return launch32<D, k()>(a, cfg, stream); });
}
template int em32_launch_d<PBBSS_EM_D>(int, const EmArgs&, const EmLaunchCfg&, hipStream_t);

}  // namespace pbbss
