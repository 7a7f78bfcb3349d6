// extern "C" boundary of the polyphase resampler and STOI (include/pbbss.h, section XI; kernels:
// stoi.hip): argument validation and the workspace.  No device code lives here.
#include "handle.hpp"
#include "stoi.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

PBBSS_API int pbbss_resample_poly(pbbss_handle_t h, const void* x, int is_f64, int64_t rows,
                                  int64_t N, int up, int down, const double* window, int taps,
                                  double* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !window || !out || x == out || rows < 1 || N < 1 || up < 1 || down < 1 ||
      taps < 1 || taps % 2 == 0)
    return PBBSS_ERR_INVALID_ARG;
  if (rows > pbbss::kStoiMaxRows || N > pbbss::kStoiMaxLength ||
      pbbss::resample_length(N, up, down) > pbbss::kStoiMaxLength)
    return PBBSS_ERR_UNSUPPORTED;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_resample_poly(x, is_f64, rows, N, up, down, window, (taps - 1) / 2, out,
                                     as_stream(stream));
}

PBBSS_API int pbbss_stoi(pbbss_handle_t h, const double* x, const double* y, int64_t outer,
                         int64_t inner, int64_t N10, int64_t x_outer_stride,
                         int64_t x_inner_stride, int64_t y_outer_stride, int64_t y_inner_stride,
                         double* out, int32_t* out_frames, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !y || !out || outer < 1 || inner < 1 || N10 < 1 || x_outer_stride < 0 ||
      x_inner_stride < 0 || y_outer_stride < 0 || y_inner_stride < 0)
    return PBBSS_ERR_INVALID_ARG;
  if (outer > pbbss::kStoiMaxRows || inner > pbbss::kStoiMaxRows ||
      outer * inner > pbbss::kStoiMaxRows || N10 > pbbss::kStoiMaxLength)
    return PBBSS_ERR_UNSUPPORTED;
  pbbss::StoiWork w{};
  const int rc = pbbss::carve(h->work, [&](pbbss::Carver& c) {
    pbbss::stoi_workspace(c, outer * inner, N10, &w);
  });
  if (rc != PBBSS_OK) return rc;
  const pbbss::StoiRows g{x,  y, outer, inner, N10, x_outer_stride, x_inner_stride,
                          y_outer_stride, y_inner_stride};
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_stoi(g, w, out, out_frames, as_stream(stream));
}
