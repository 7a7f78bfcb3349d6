// extern "C" boundary of the WPE dereverberation (include/pbbss.h, XIII; kernels: wpe.hip):
// argument validation, the workspace and the chain of launches.  No device code lives here.
#include "handle.hpp"
#include "wpe.hpp"
#include "wpe_online.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion, pbbss::WpeFrames, pbbss::WpeWork;

namespace {
int check_frames(const void* y, int64_t B, int D, int64_t T) {
  if (!y || B < 1 || T < 1 || D < 1) return PBBSS_ERR_INVALID_ARG;
  if (D > pbbss::kWpeMaxD || T > INT32_MAX / 4) return PBBSS_ERR_UNSUPPORTED;
  return PBBSS_OK;
}
int check_taps(int D, int taps, int delay) {
  if (taps < 1 || delay < 0) return PBBSS_ERR_INVALID_ARG;
  if (taps > pbbss::kWpeMaxM / D || delay > INT32_MAX / 4) return PBBSS_ERR_UNSUPPORTED;
  return PBBSS_OK;
}
// problems per chunk: the span sums of a chunk stay below kWpeWorkspaceCap and every grid of the
// chain (at most spans workgroups, 256 finishing threads per tile, per problem) fits 31 bits
int64_t chunk_size(int64_t B, int D, int64_t T, int taps) {
  const size_t per = (size_t)pbbss::wpe_spans(T) * pbbss::wpe_tiles(D, taps) * 256 * 16;
  int64_t n = (int64_t)(pbbss::kWpeWorkspaceCap / per);
  const int64_t grid = INT32_MAX / ((T + 127) / 128 + pbbss::wpe_tiles(D, taps));
  if (n > grid) n = grid;
  if (n < 1) n = 1;
  return n < B ? n : B;
}
WpeFrames frames(const void* y, int c128, int D, int64_t T, int64_t sb, int64_t sd, int64_t st) {
  return WpeFrames{y, c128, T, sb, sd, st, D};
}
const void* offset(const void* p, int c128, int64_t elements) {
  return static_cast<const char*>(p) + elements * (c128 ? 16 : 8);
}
// the floats of one chunk; `full`: everything pbbss_wpe needs, else only the span sums
void pieces(pbbss::Carver& c, WpeWork& w, int64_t n, int D, int64_t T, int taps, bool full) {
  const size_t M = (size_t)D * taps;
  w.part = c.take<double>((size_t)n * pbbss::wpe_spans(T) * pbbss::wpe_tiles(D, taps) * 512);
  if (!full) return;
  w.raw = c.take<double>((size_t)n * T);
  w.power = c.take<double>((size_t)n * T);
  w.inv = c.take<double>((size_t)n * T);
  w.pmax = c.take<double>((size_t)n);
  w.R = c.take<double>((size_t)n * M * M * 2);
  w.P = c.take<double>((size_t)n * M * D * 2);
  w.G = c.take<double>((size_t)n * M * D * 2);
}
}  // namespace

PBBSS_API int pbbss_wpe(pbbss_handle_t h, const void* y, int y_is_c128, int64_t B, int D,
                        int64_t T, int64_t stride_b, int64_t stride_d, int64_t stride_t, int taps,
                        int delay, int iterations, int64_t psd_context, int statistics_mode,
                        void* out_x, int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  int rc = check_frames(y, B, D, T);
  if (!h || !out_x || !out_status || rc == PBBSS_ERR_INVALID_ARG || iterations < 1 ||
      psd_context < -1 ||
      (statistics_mode != PBBSS_WPE_STATISTICS_FULL && statistics_mode != PBBSS_WPE_STATISTICS_VALID))
    return PBBSS_ERR_INVALID_ARG;
  if (rc == PBBSS_OK) rc = check_taps(D, taps, delay);
  if (rc != PBBSS_OK) return rc;
  if (h->cfg.lds_limit && h->cfg.lds_limit < pbbss::kWpeLds) return PBBSS_ERR_LDS_CAPACITY;
  const int64_t n = chunk_size(B, D, T, taps);
  WpeWork w{};
  rc = pbbss::carve(h->work, [&](pbbss::Carver& c) { pieces(c, w, n, D, T, taps, true); });
  if (rc != PBBSS_OK) return rc;
  hipStream_t s = as_stream(stream);
  TimedRegion tr(h, s);
  const WpeFrames none = frames(nullptr, 0, D, T, 0, 0, 0);
  for (int64_t b0 = 0; b0 < B; b0 += n) {
    const int64_t nb = B - b0 < n ? B - b0 : n;
    const WpeFrames yc = frames(offset(y, y_is_c128, b0 * stride_b), y_is_c128, D, T, stride_b,
                                stride_d, stride_t);
    void* xc = const_cast<void*>(offset(out_x, y_is_c128, b0 * stride_b));
    rc = pbbss::launch_wpe_inverse_power(yc, nullptr, nb, psd_context, w.raw, w.power, w.inv,
                                         w.pmax, s);
    for (int it = 0; it < iterations && rc == PBBSS_OK; ++it) {
      const bool last = it == iterations - 1;
      rc = pbbss::launch_wpe_correlations(yc, nb, w.inv, taps, delay,
                                          statistics_mode == PBBSS_WPE_STATISTICS_VALID, w.part,
                                          w.R, w.P, s);
      if (rc == PBBSS_OK)
        rc = pbbss::launch_wpe_solve(w.R, w.P, w.pmax, nb, D, taps, w.G, out_status + b0, s);
      if (rc == PBBSS_OK)
        rc = pbbss::launch_wpe_apply(yc, nb, w.G, taps, delay, last ? xc : nullptr,
                                     last ? nullptr : w.raw, s);
      if (rc == PBBSS_OK && !last)
        rc = pbbss::launch_wpe_inverse_power(none, w.raw, nb, psd_context, nullptr, w.power, w.inv,
                                             w.pmax, s);
    }
    if (rc != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}

PBBSS_API int pbbss_wpe_power_inverse(pbbss_handle_t h, const void* y, int y_is_c128, int64_t B,
                                      int D, int64_t T, int64_t stride_b, int64_t stride_d,
                                      int64_t stride_t, int64_t psd_context, double* out_power,
                                      double* out_inverse_power, void* stream) {
  DeviceGuard device_guard(h);
  const int rc = check_frames(y, B, D, T);
  if (!h || !out_power || rc == PBBSS_ERR_INVALID_ARG || psd_context < -1)
    return PBBSS_ERR_INVALID_ARG;
  if (rc != PBBSS_OK || B > INT32_MAX / ((T + 255) / 256)) return PBBSS_ERR_UNSUPPORTED;
  double* raw = out_power;  // smoothing reads its neighbours: it needs the raw power elsewhere
  if (psd_context > 0 && !(raw = static_cast<double*>(h->work.grow((size_t)B * T * 8))))
    return PBBSS_ERR_HIP;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_wpe_inverse_power(frames(y, y_is_c128, D, T, stride_b, stride_d, stride_t),
                                         nullptr, B, psd_context, raw, out_power,
                                         out_inverse_power, nullptr, as_stream(stream));
}

PBBSS_API int pbbss_wpe_correlations(pbbss_handle_t h, const void* y, int y_is_c128, int64_t B,
                                     int D, int64_t T, int64_t stride_b, int64_t stride_d,
                                     int64_t stride_t, const double* inverse_power, int taps,
                                     int delay, int statistics_mode, void* out_R, void* out_P,
                                     void* stream) {
  DeviceGuard device_guard(h);
  int rc = check_frames(y, B, D, T);
  if (!h || !inverse_power || !out_R || !out_P || rc == PBBSS_ERR_INVALID_ARG ||
      (statistics_mode != PBBSS_WPE_STATISTICS_FULL && statistics_mode != PBBSS_WPE_STATISTICS_VALID))
    return PBBSS_ERR_INVALID_ARG;
  if (rc == PBBSS_OK) rc = check_taps(D, taps, delay);
  if (rc != PBBSS_OK) return rc;
  if (h->cfg.lds_limit && h->cfg.lds_limit < pbbss::kWpeLds) return PBBSS_ERR_LDS_CAPACITY;
  const int64_t n = chunk_size(B, D, T, taps);
  WpeWork w{};
  rc = pbbss::carve(h->work, [&](pbbss::Carver& c) { pieces(c, w, n, D, T, taps, false); });
  if (rc != PBBSS_OK) return rc;
  TimedRegion tr(h, as_stream(stream));
  const int64_t M = (int64_t)D * taps;
  for (int64_t b0 = 0; b0 < B && rc == PBBSS_OK; b0 += n)
    rc = pbbss::launch_wpe_correlations(
        frames(offset(y, y_is_c128, b0 * stride_b), y_is_c128, D, T, stride_b, stride_d, stride_t),
        B - b0 < n ? B - b0 : n, inverse_power + b0 * T, taps, delay,
        statistics_mode == PBBSS_WPE_STATISTICS_VALID, w.part,
        static_cast<double*>(out_R) + b0 * M * M * 2, static_cast<double*>(out_P) + b0 * M * D * 2,
        as_stream(stream));
  return rc;
}

PBBSS_API int pbbss_wpe_filter_matrix(pbbss_handle_t h, const void* R, const void* P, int64_t B,
                                      int D, int taps, void* out_G, int32_t* out_status,
                                      void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !R || !P || !out_G || !out_status || B < 1 || D < 1 || taps < 1)
    return PBBSS_ERR_INVALID_ARG;
  if (D > pbbss::kWpeMaxD || taps > pbbss::kWpeMaxM / D || B > INT32_MAX)
    return PBBSS_ERR_UNSUPPORTED;
  if (h->cfg.lds_limit && h->cfg.lds_limit < pbbss::kWpeLds) return PBBSS_ERR_LDS_CAPACITY;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_wpe_solve(static_cast<const double*>(R), static_cast<const double*>(P),
                                 nullptr, B, D, taps, static_cast<double*>(out_G), out_status,
                                 as_stream(stream));
}

PBBSS_API int pbbss_wpe_apply_filter(pbbss_handle_t h, const void* y, int y_is_c128, int64_t B,
                                     int D, int64_t T, int64_t stride_b, int64_t stride_d,
                                     int64_t stride_t, const void* G, int taps, int delay,
                                     void* out_x, void* stream) {
  DeviceGuard device_guard(h);
  int rc = check_frames(y, B, D, T);
  if (!h || !G || !out_x || rc == PBBSS_ERR_INVALID_ARG) return PBBSS_ERR_INVALID_ARG;
  if (rc == PBBSS_OK) rc = check_taps(D, taps, delay);
  if (rc != PBBSS_OK) return rc;
  if (B > INT32_MAX / ((T + 255) / 256)) return PBBSS_ERR_UNSUPPORTED;
  if (h->cfg.lds_limit && h->cfg.lds_limit < pbbss::kWpeLds) return PBBSS_ERR_LDS_CAPACITY;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_wpe_apply(frames(y, y_is_c128, D, T, stride_b, stride_d, stride_t), B,
                                 static_cast<const double*>(G), taps, delay, out_x, nullptr,
                                 as_stream(stream));
}

PBBSS_API int pbbss_wpe_online(pbbss_handle_t h, const void* y, int y_is_c128, int64_t B, int D,
                               int64_t T, int64_t stride_b, int64_t stride_d, int64_t stride_t,
                               int taps, int delay, double alpha, const double* power_estimate,
                               void* inv_cov, void* filter_taps, void* history,
                               int64_t* frames_seen, void* out_x, int32_t* out_status,
                               void* stream) {
  DeviceGuard device_guard(h);
  int rc = check_frames(y, B, D, T);
  if (!h || !inv_cov || !filter_taps || !history || !frames_seen || !out_x || !out_status ||
      rc == PBBSS_ERR_INVALID_ARG || taps < 1 || delay < 0 || !(alpha > 0.0 && alpha <= 1.0))
    return PBBSS_ERR_INVALID_ARG;
  if (rc == PBBSS_OK) rc = check_taps(D, taps, delay);
  if (rc != PBBSS_OK) return rc;
  if (B > INT32_MAX || (int64_t)D * ((int64_t)taps + delay) > pbbss::kWpeOnlineMaxRing)
    return PBBSS_ERR_UNSUPPORTED;
  if (h->cfg.lds_limit && h->cfg.lds_limit < pbbss::kWpeLds) return PBBSS_ERR_LDS_CAPACITY;
  TimedRegion tr(h, as_stream(stream));
  const pbbss::WpeOnlineState st{power_estimate, static_cast<double*>(inv_cov),
                                 static_cast<double*>(filter_taps), static_cast<double*>(history),
                                 frames_seen};
  return pbbss::launch_wpe_online(frames(y, y_is_c128, D, T, stride_b, stride_d, stride_t), B, taps,
                                  delay, alpha, st, out_x, out_status, as_stream(stream));
}
