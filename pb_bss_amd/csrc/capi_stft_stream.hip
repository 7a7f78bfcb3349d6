// extern "C" boundary of the streaming STFT edge (include/pbbss_stream.h; kernels:
// stft_stream.hip): argument validation and the launch.  The handle names the device and its LDS
// limit; nothing is carved from it.  No device code lives here.
#include "handle.hpp"
#include "pbbss_stream.h"
#include "stft_stream.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

PBBSS_API int pbbss_stft_stream(pbbss_handle_t h, const void* x, int x_is_f64, int64_t C, int64_t n,
                                const double* hist_in, double* hist_out, int64_t samples_seen,
                                int64_t frames_seen, int m, int flush, int size, int shift,
                                int window_length, const double* window, int fading, int out_layout,
                                int out_is_c128, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !hist_in || !hist_out || hist_in == hist_out || !window || C <= 0 || n < 0 || m < 0 ||
      samples_seen < 0 || frames_seen < 0 || (n > 0 && !x) || (m > 0 && !out) || shift < 1 ||
      window_length < 1 || (flush && n != 0))
    return PBBSS_ERR_INVALID_ARG;
  if (fading && window_length < shift) return PBBSS_ERR_INVALID_ARG;
  if (C > 65535 || samples_seen > INT64_MAX / 4 || frames_seen > INT32_MAX)
    return PBBSS_ERR_UNSUPPORTED;
  const int hist_len = window_length > 1 ? window_length - 1 : 1;
  const int fade = fading ? window_length - shift : 0;
  // position of the first sample of frame frames_seen, relative to the first sample of the block
  const int64_t base = frames_seen * shift - fade - samples_seen;
  if (m > 0 && base < -(int64_t)hist_len) return PBBSS_ERR_INVALID_ARG;  // a frame was skipped
  if (!flush) {
    // exactly the frames that end inside the block
    const int64_t room = n - base - window_length;  // >= 0: frame frames_seen is complete
    const int64_t complete = room < 0 ? 0 : room / shift + 1;
    if (complete != m) return PBBSS_ERR_INVALID_ARG;
    if (n == 0) return PBBSS_OK;  // (then m == 0) nothing moves
  }
  const int64_t lo = -(samples_seen < hist_len ? samples_seen : (int64_t)hist_len);
  TimedRegion tr(h, as_stream(stream));
  const pbbss::StftStreamArgs a{x, x_is_f64, C, n, hist_in, hist_out, hist_len, lo, base, m,
                                flush ? 1 : 0, size, shift, window_length, window, out_layout,
                                out_is_c128, out};
  return pbbss::launch_stft_stream(a, h->cfg.lds_limit, as_stream(stream));
}

PBBSS_API int pbbss_istft_stream(pbbss_handle_t h, const void* X, int x_is_c128, int64_t rows, int m,
                                 int64_t stride_r, int64_t stride_t, int64_t stride_f, int size,
                                 int shift, int window_length, const double* synthesis_window,
                                 double* tail, int skip, double* out, int64_t n_out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !X || !synthesis_window || rows <= 0 || m < 1 || shift < 1 || window_length < shift ||
      window_length % shift != 0 || (!tail && window_length != shift) || skip < 0 ||
      skip > window_length - shift)
    return PBBSS_ERR_INVALID_ARG;
  const int64_t want = (int64_t)m * shift - skip;
  if (n_out != (want > 0 ? want : 0) || (n_out > 0 && !out)) return PBBSS_ERR_INVALID_ARG;
  if (rows > 65535) return PBBSS_ERR_UNSUPPORTED;
  TimedRegion tr(h, as_stream(stream));
  const pbbss::IstftStreamArgs a{X, x_is_c128, rows, m, stride_r, stride_t, stride_f, size, shift,
                                 window_length, synthesis_window, tail, skip, out, n_out};
  return pbbss::launch_istft_stream(a, h->cfg.lds_limit, as_stream(stream));
}
