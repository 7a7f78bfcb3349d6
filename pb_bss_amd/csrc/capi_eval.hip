// extern "C" boundary of the evaluation metrics (include/pbbss.h, section V; kernels: eval.hip):
// argument validation and the workspace of the span partials.  No device code lives here.
#include "handle.hpp"
#include "eval.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

static bool eval_dtype_ok(int dtype) { return dtype >= PBBSS_EVAL_F32 && dtype <= PBBSS_EVAL_C128; }

static int64_t eval_reals(int dtype) { return pbbss::eval_is_complex(dtype) ? 2 : 1; }

// is p a multiple of the size of one real of the signal (4 or 8 bytes)?
static bool eval_aligned(const void* p, bool is_f64) {
  return reinterpret_cast<uintptr_t>(p) % (is_f64 ? 8u : 4u) == 0;
}

PBBSS_API int pbbss_signal_power(pbbss_handle_t h, const void* x, int dtype, int64_t rows,
                                 int64_t length, int64_t row_stride, double* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !out || !eval_dtype_ok(dtype) || rows < 1 || length < 1 || row_stride < 0 ||
      !eval_aligned(x, pbbss::eval_is_f64(dtype)))
    return PBBSS_ERR_INVALID_ARG;
  if (length > INT64_MAX / 2 || !pbbss::eval_grid_ok(rows, length * eval_reals(dtype)))
    return PBBSS_ERR_UNSUPPORTED;
  double* work = static_cast<double*>(
      h->work.grow(pbbss::signal_power_work(rows, length, dtype) * sizeof(double)));
  if (!work) return PBBSS_ERR_HIP;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_signal_power(x, dtype, rows, length, row_stride, work, out,
                                    as_stream(stream));
}

PBBSS_API int pbbss_si_sdr(pbbss_handle_t h, const void* reference, const void* estimation,
                           int is_f64, int64_t B, int Kr, int Ke, int64_t N,
                           int64_t ref_batch_stride, int64_t ref_row_stride,
                           int64_t est_batch_stride, int64_t est_row_stride, double* out,
                           void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !reference || !estimation || !out || B < 1 || Kr < 1 || Ke < 1 || N < 1 ||
      ref_batch_stride < 0 || ref_row_stride < 0 || est_batch_stride < 0 || est_row_stride < 0 ||
      !eval_aligned(reference, is_f64 != 0) || !eval_aligned(estimation, is_f64 != 0))
    return PBBSS_ERR_INVALID_ARG;
  if (Kr > pbbss::kEvalMaxRows || Ke > pbbss::kEvalMaxRows || !pbbss::eval_grid_ok(B, N))
    return PBBSS_ERR_UNSUPPORTED;
  double* work =
      static_cast<double*>(h->work.grow(pbbss::si_sdr_work(B, Kr, Ke, N) * sizeof(double)));
  if (!work) return PBBSS_ERR_HIP;
  pbbss::EvalRows g{};
  g.ref = reference;
  g.est = estimation;
  g.B = B;
  g.N = N;
  g.ref_batch = ref_batch_stride;
  g.ref_row = ref_row_stride;
  g.est_batch = est_batch_stride;
  g.est_row = est_row_stride;
  g.Kr = Kr;
  g.Ke = Ke;
  g.is_f64 = is_f64 != 0;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_si_sdr(g, work, out, as_stream(stream));
}

// the two span-partial arrays of an sxr call: `rows_images` and `rows_noise` rows of N samples
static int sxr_work(pbbss_handle_t h, int64_t rows_images, int64_t rows_noise, int64_t N, int dtype,
                    double** work_images, double** work_noise) {
  return pbbss::carve(h->work, [&](pbbss::Carver& c) {
    *work_images = c.take<double>(pbbss::signal_power_work(rows_images, N, dtype));
    *work_noise = c.take<double>(pbbss::signal_power_work(rows_noise, N, dtype));
  });
}

PBBSS_API int pbbss_output_sxr(pbbss_handle_t h, const void* contributions, const void* noise,
                               int dtype, int64_t B, int Ks, int Kt, int64_t N,
                               int average_sources, double* out_sxr, int64_t* out_selection,
                               double* out_mean, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !contributions || !noise || !out_sxr || !out_selection || !eval_dtype_ok(dtype) ||
      B < 1 || Ks < 1 || Kt < 1 || N < 1 || (average_sources && !out_mean) ||
      !eval_aligned(contributions, pbbss::eval_is_f64(dtype)) ||
      !eval_aligned(noise, pbbss::eval_is_f64(dtype)))
    return PBBSS_ERR_INVALID_ARG;
  if (Ks > Kt) return PBBSS_ERR_INVALID_ARG;  // no selection exists
  if (Kt > pbbss::kSxrMaxTargets) return PBBSS_ERR_UNSUPPORTED;
  if (N > INT64_MAX / 2 || B > INT32_MAX / (Ks * Kt) ||
      !pbbss::eval_grid_ok(B * Ks * Kt, N * eval_reals(dtype)))
    return PBBSS_ERR_UNSUPPORTED;
  double *wi = nullptr, *wn = nullptr;
  const int rc = sxr_work(h, B * Ks * Kt, B * Kt, N, dtype, &wi, &wn);
  if (rc != PBBSS_OK) return rc;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_output_sxr(contributions, noise, dtype, B, Ks, Kt, N, average_sources, wi,
                                  wn, out_sxr, out_selection, out_mean, as_stream(stream));
}

PBBSS_API int pbbss_input_sxr(pbbss_handle_t h, const void* images, const void* noise, int dtype,
                              int64_t B, int K, int D, int64_t N, int average_sources,
                              int average_channels, double* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !images || !noise || !out || !eval_dtype_ok(dtype) || B < 1 || K < 1 || D < 1 ||
      N < 1 || !eval_aligned(images, pbbss::eval_is_f64(dtype)) ||
      !eval_aligned(noise, pbbss::eval_is_f64(dtype)))
    return PBBSS_ERR_INVALID_ARG;
  if (K > pbbss::kSxrMaxSources || D > pbbss::kSxrMaxSensors) return PBBSS_ERR_UNSUPPORTED;
  if (N > INT64_MAX / 2 || B > INT32_MAX / (K * D) ||
      !pbbss::eval_grid_ok(B * K * D, N * eval_reals(dtype)))
    return PBBSS_ERR_UNSUPPORTED;
  double *wi = nullptr, *wn = nullptr;
  const int rc = sxr_work(h, B * K * D, B * D, N, dtype, &wi, &wn);
  if (rc != PBBSS_OK) return rc;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_input_sxr(images, noise, dtype, B, K, D, N, average_sources,
                                 average_channels, wi, wn, out, as_stream(stream));
}
