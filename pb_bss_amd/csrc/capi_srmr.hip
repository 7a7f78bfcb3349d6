// extern "C" boundary of the gammatone filterbank and SRMR (include/pbbss.h, section X; kernels:
// srmr.hip): argument validation and the two workspaces.  No device code lives here.
#include "handle.hpp"
#include "srmr.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

// rows, row length and channel count of one call: PBBSS_OK, or the code to return
static int srmr_shape(int64_t rows, int64_t N, int n) {
  if (rows < 1 || N < 1) return PBBSS_ERR_INVALID_ARG;
  if (n < 1 || n > pbbss::kSrmrMaxChannels || N > pbbss::kSrmrMaxLength) return PBBSS_ERR_UNSUPPORTED;
  // rows is a grid y extent, rows * n a grid x extent
  if (rows > 65535) return PBBSS_ERR_UNSUPPORTED;
  return PBBSS_OK;
}

PBBSS_API int pbbss_srmr_vad(pbbss_handle_t h, const void* x, int is_f64, int64_t rows, int64_t N,
                             int sample_rate, double* out, int32_t* out_lengths, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !out || !out_lengths || x == out) return PBBSS_ERR_INVALID_ARG;
  const int rc = srmr_shape(rows, N, 1);
  if (rc != PBBSS_OK) return rc;
  if (sample_rate < pbbss::kSrmrMinSampleRate) return PBBSS_ERR_UNSUPPORTED;
  int32_t* right = static_cast<int32_t*>(h->work.grow((size_t)(rows * N) * sizeof(int32_t)));
  if (!right) return PBBSS_ERR_HIP;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_srmr_vad(x, is_f64, rows, N, sample_rate, right, out, out_lengths,
                                as_stream(stream));
}

PBBSS_API int pbbss_gammatone(pbbss_handle_t h, const void* x, int is_f64, int64_t rows, int64_t N,
                              const int32_t* lengths, int n, const double* coef, double* out,
                              void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !coef || !out || x == out) return PBBSS_ERR_INVALID_ARG;
  const int rc = srmr_shape(rows, N, n);
  if (rc != PBBSS_OK) return rc;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_gammatone(x, is_f64, rows, N, lengths, n, coef, out, as_stream(stream));
}

PBBSS_API int pbbss_srmr_energies(pbbss_handle_t h, const void* analytic, int64_t rows, int64_t N,
                                  const int32_t* lengths, int n, int sample_rate,
                                  const double* coef, double* out_means, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !analytic || !coef || !out_means) return PBBSS_ERR_INVALID_ARG;
  const int rc = srmr_shape(rows, N, n);
  if (rc != PBBSS_OK) return rc;
  if (sample_rate < pbbss::kSrmrMinSampleRate) return PBBSS_ERR_UNSUPPORTED;
  double* weights = static_cast<double*>(h->work.grow((size_t)(rows * N) * sizeof(double)));
  if (!weights) return PBBSS_ERR_HIP;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_srmr_energies(analytic, rows, N, lengths, n, sample_rate, coef, weights,
                                     out_means, as_stream(stream));
}

PBBSS_API int pbbss_srmr_score(pbbss_handle_t h, const double* means, int64_t rows, int n,
                               const double* erbs, const double* cutoffs, double* out,
                               void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !means || !erbs || !cutoffs || !out) return PBBSS_ERR_INVALID_ARG;
  const int rc = srmr_shape(rows, 1, n);
  if (rc != PBBSS_OK) return rc;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_srmr_score(means, rows, n, erbs, cutoffs, out, as_stream(stream));
}
