// Host-side entry points of the complex-Bingham kernels (cbmm_inst.hip), one per compiled D.
#pragma once
#include "cbmm.hpp"
#include "em_launch.hpp"

namespace pbbss {

#define PBBSS_CB_DECL(d)                                                                      \
  int cb_launch_d##d(int K, int y_is_c128, const BinghamArgs&, const EmLaunchCfg&, hipStream_t); \
  int cb_solve_launch_d##d(const double* s, int64_t N, double eps, double maxc, double* lam,   \
                           int32_t* status, int num_cu, hipStream_t stream);
PBBSS_CB_DECL(2)
PBBSS_CB_DECL(3)
PBBSS_CB_DECL(4)
PBBSS_CB_DECL(5)
PBBSS_CB_DECL(6)
PBBSS_CB_DECL(7)
PBBSS_CB_DECL(8)
#undef PBBSS_CB_DECL

inline int cb_launch(int D, int K, int y_is_c128, const BinghamArgs& a, const EmLaunchCfg& cfg,
                     hipStream_t s) {
  switch (D) {
    case 2: return cb_launch_d2(K, y_is_c128, a, cfg, s);
    case 3: return cb_launch_d3(K, y_is_c128, a, cfg, s);
    case 4: return cb_launch_d4(K, y_is_c128, a, cfg, s);
    case 5: return cb_launch_d5(K, y_is_c128, a, cfg, s);
    case 6: return cb_launch_d6(K, y_is_c128, a, cfg, s);
    case 7: return cb_launch_d7(K, y_is_c128, a, cfg, s);
    case 8: return cb_launch_d8(K, y_is_c128, a, cfg, s);
    default: return PBBSS_ERR_UNSUPPORTED;
  }
}

inline int cb_solve_launch(int D, const double* s_in, int64_t N, double eps, double maxc,
                           double* lam, int32_t* status, int num_cu, hipStream_t s) {
  switch (D) {
    case 2: return cb_solve_launch_d2(s_in, N, eps, maxc, lam, status, num_cu, s);
    case 3: return cb_solve_launch_d3(s_in, N, eps, maxc, lam, status, num_cu, s);
    case 4: return cb_solve_launch_d4(s_in, N, eps, maxc, lam, status, num_cu, s);
    case 5: return cb_solve_launch_d5(s_in, N, eps, maxc, lam, status, num_cu, s);
    case 6: return cb_solve_launch_d6(s_in, N, eps, maxc, lam, status, num_cu, s);
    case 7: return cb_solve_launch_d7(s_in, N, eps, maxc, lam, status, num_cu, s);
    case 8: return cb_solve_launch_d8(s_in, N, eps, maxc, lam, status, num_cu, s);
    default: return PBBSS_ERR_UNSUPPORTED;
  }
}

}  // namespace pbbss
