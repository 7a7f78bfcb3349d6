// extern "C" boundary of the complex circular-symmetric Gaussian (include/pbbss.h, XII; kernels:
// ccsg.hip): argument validation and the workspace.  No device code lives here.
#include "handle.hpp"
#include "ccsg.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

namespace {
// one workgroup per (batch item, ccsg_frames(D) frames): the grid must fit 31 bits
bool grid_ok(int64_t B, int64_t N, int D) {
  const int64_t tiles = (N + pbbss::ccsg_frames(D) - 1) / pbbss::ccsg_frames(D);
  return B <= INT32_MAX / tiles;
}
}  // namespace

PBBSS_API int pbbss_ccsg_fit(pbbss_handle_t h, const void* y, int y_is_c128, int64_t B, int64_t N,
                             int D, int K, const void* saliency, int saliency_is_f64,
                             double floor, void* out_covariance, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !out_covariance || B < 1 || N < 1 || K < 1 || (!saliency && K != 1))
    return PBBSS_ERR_INVALID_ARG;
  if (D < 1 || D > pbbss::kCcsgMaxD || K > INT32_MAX / 1024 || !grid_ok(B, N, D))
    return PBBSS_ERR_UNSUPPORTED;
  // the finishing kernel: one thread per entry of the lower triangles, 256 per workgroup
  if (B * K > INT32_MAX / (D * (D + 1) / 2) * (int64_t)256) return PBBSS_ERR_UNSUPPORTED;
  if (h->cfg.lds_limit && h->cfg.lds_limit < pbbss::kCcsgLds) return PBBSS_ERR_LDS_CAPACITY;
  const size_t np = pbbss::ccsg_fit_partials(B, N, D, K);
  void* w = h->work.grow(np * 16);
  if (!w) return PBBSS_ERR_HIP;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_ccsg_fit(y, y_is_c128, B, N, D, K, saliency, saliency_is_f64, floor,
                                static_cast<double*>(w), static_cast<double*>(out_covariance),
                                as_stream(stream));
}

PBBSS_API int pbbss_ccsg_log_pdf(pbbss_handle_t h, const void* y, int y_is_c128, int64_t B,
                                 int64_t N, int D, int K, const void* covariance,
                                 double* out_log_pdf, double* out_log_det, int32_t* out_status,
                                 void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !covariance || !out_log_pdf || !out_status || B < 1 || N < 1 || K < 1)
    return PBBSS_ERR_INVALID_ARG;
  if (D < 1 || D > pbbss::kCcsgMaxD || !grid_ok(B, N, D)) return PBBSS_ERR_UNSUPPORTED;
  if (h->cfg.lds_limit && h->cfg.lds_limit < pbbss::kCcsgLds) return PBBSS_ERR_LDS_CAPACITY;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_ccsg_log_pdf(y, y_is_c128, B, N, D, K,
                                    static_cast<const double*>(covariance), out_log_pdf,
                                    out_log_det, out_status, as_stream(stream));
}
