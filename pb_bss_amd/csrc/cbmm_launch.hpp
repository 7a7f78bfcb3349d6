// Host-side entry points of the complex-Bingham kernels (cbmm_inst.hip), one per compiled D.
#pragma once
#include "cbmm.hpp"
#include "em_launch.hpp"

namespace pbbss {

template <int D> int cb_launch_d(int K, int y_is_c128, const BinghamArgs&, const EmLaunchCfg&, hipStream_t);
template <int D> int cb_solve_launch_d(const double* s, int64_t N, double eps, double maxc, double* lam,
                                       int32_t* status, int num_cu, hipStream_t stream);

#ifndef PBBSS_EM_D  // see em_launch.hpp
inline int cb_launch(int D, int K, int y_is_c128, const BinghamArgs& a, const EmLaunchCfg& cfg,
                     hipStream_t s) {
  return dispatch_range<2, 8>(D, [&](auto d) { return cb_launch_d<d()>(K, y_is_c128, a, cfg, s); });
}

inline int cb_solve_launch(int D, const double* s_in, int64_t N, double eps, double maxc,
                           double* lam, int32_t* status, int num_cu, hipStream_t s) {
  return dispatch_range<2, 8>(D, [&](auto d) {
    return cb_solve_launch_d<d()>(s_in, N, eps, maxc, lam, status, num_cu, s);
  });
}
#endif

}  // namespace pbbss
