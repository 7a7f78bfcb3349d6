// Complex-Bingham mixture EM kernel and the Bingham parameter solve, one translation unit per
// sensor count D (compiled with -DPBBSS_EM_D=<D>), like cw_inst.hip.
#include "cbmm.hpp"
#include "cbmm_launch.hpp"
#include "em_launch.hpp"

#ifndef PBBSS_EM_D
#error "compile with -DPBBSS_EM_D=<sensors>"
#endif

namespace pbbss {

template <int D, int K, typename YS, bool SPILL>
static int cb_launch_variant(BinghamArgs ba, const EmLaunchCfg& cfg, hipStream_t stream) {
  using Kern = BinghamKernel<D, K, YS, SPILL>;
  const size_t lds = Kern::lds_bytes(ba.em.T);
  if (lds > cfg.lds_limit) return PBBSS_ERR_LDS_CAPACITY;
  auto kfn = cbmm_em_kernel<D, K, YS, SPILL>;
  int occ = blocks_per_cu(kfn, kEmThreads, lds);
  if (occ < 0) return PBBSS_ERR_HIP;
  if (occ < 1) occ = 1;
  int64_t grid = (int64_t)cfg.num_cu * occ;
  if (grid > ba.em.B) grid = ba.em.B;
  if (SPILL) {  // frame arrays of each workgroup in HBM scratch (cw_inst.hip: cw_launch_variant)
    ba.em.scratch_stride = Kern::Base::scratch_bytes(ba.em.T);
    ba.em.scratch =
        static_cast<char*>(cfg.get_scratch(cfg.scratch_ctx, ba.em.scratch_stride * grid));
    if (!ba.em.scratch) return PBBSS_ERR_HIP;
  }
  hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(kEmThreads), lds, stream, ba);
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

// frames LDS-resident when they fit, else the spilled variant (long utterances)
template <int D, int K, typename YS>
static int cb_launch_one(const BinghamArgs& ba, const EmLaunchCfg& cfg, hipStream_t stream) {
  if (BinghamKernel<D, K, YS, false>::lds_bytes(ba.em.T) > cfg.lds_limit)
    return cb_launch_variant<D, K, YS, true>(ba, cfg, stream);
  return cb_launch_variant<D, K, YS, false>(ba, cfg, stream);
}

template <int D>
int cb_launch_d(int K, int y_is_c128, const BinghamArgs& ba, const EmLaunchCfg& cfg,
                hipStream_t stream) {
  return dispatch_real(y_is_c128, [&](auto y) {
    return dispatch_range<1, 4>(
        K, [&](auto k) { return cb_launch_one<D, k(), decltype(y)>(ba, cfg, stream); });
  });
}
template int cb_launch_d<PBBSS_EM_D>(int, int, const BinghamArgs&, const EmLaunchCfg&, hipStream_t);

template <int D>
int cb_solve_launch_d(const double* s, int64_t N, double eps, double maxc, double* lam,
                      int32_t* status, int num_cu, hipStream_t stream) {
  int64_t grid = (int64_t)num_cu * 8;
  if (grid > N) grid = N;
  hipLaunchKernelGGL(cbingham_find_eigenvalues_kernel<D>, dim3((unsigned)grid), dim3(kWave), 0,
                     stream, s, N, eps, maxc, lam, status);
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}
template int cb_solve_launch_d<PBBSS_EM_D>(const double*, int64_t, double, double, double*, int32_t*,
                                           int, hipStream_t);

}  // namespace pbbss
