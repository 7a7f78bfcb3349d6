// extern "C" boundary of the frame-recursive cACGMM mask estimator (include/pbbss.h, XV; kernel:
// online_cacgmm.hip): argument validation and the launch.  No device code lives here.
#include "handle.hpp"
#include "online_cacgmm.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

PBBSS_API int pbbss_online_cacgmm(pbbss_handle_t h, const void* y, int y_is_c128, int64_t B, int D,
                                  int K, int64_t T, int64_t stride_b, int64_t stride_d,
                                  int64_t stride_t, double alpha, double affiliation_eps,
                                  int update_weight, void* precision, double* log_determinant,
                                  double* count, double* weight, int64_t* frames_seen,
                                  double* out_affiliation, double* out_quadratic_form,
                                  int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !precision || !log_determinant || !count || !weight || !frames_seen ||
      !out_affiliation || !out_status || B < 1 || D < 2 || K < 2 || T < 1 ||
      !(alpha > 0.0 && alpha <= 1.0) || !(affiliation_eps >= 0.0 && affiliation_eps < 0.5))
    return PBBSS_ERR_INVALID_ARG;
  if (D > pbbss::kOnlineCacgmmMaxD || K > pbbss::kOnlineCacgmmMaxK || T > INT32_MAX / 4 ||
      B > INT32_MAX)
    return PBBSS_ERR_UNSUPPORTED;
  TimedRegion tr(h, as_stream(stream));
  const pbbss::WpeFrames frames{y, y_is_c128, T, stride_b, stride_d, stride_t, D};
  const pbbss::OnlineCacgmmArgs a{K, alpha, affiliation_eps, update_weight,
                                  static_cast<double*>(precision), log_determinant, count, weight,
                                  frames_seen, out_affiliation, out_quadratic_form, out_status};
  return pbbss::launch_online_cacgmm(frames, B, a, as_stream(stream));
}
