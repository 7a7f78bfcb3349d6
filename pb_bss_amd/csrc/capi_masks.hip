// extern "C" boundary of the oracle masks (include/pbbss.h, section M; kernels: masks.hip):
// argument validation and the workspace of the threshold masks.  No device code lives here.
#include "handle.hpp"
#include "masks.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

PBBSS_API int pbbss_mask_pointwise(pbbss_handle_t h, const void* x, int x_is_c128, int mode,
                                   const pbbss_mask_geom* geom, double eps, const double* table,
                                   int64_t table_len, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !geom || !out) return PBBSS_ERR_INVALID_ARG;
  if (mode < PBBSS_MASK_IBM || mode > PBBSS_MASK_BIASED) return PBBSS_ERR_INVALID_ARG;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_mask_pointwise(x, x_is_c128, mode, *geom, eps, table, table_len, out,
                                      as_stream(stream));
}

static int mask_threshold(pbbss_handle_t h, const void* x, int x_is_c128,
                          const pbbss_mask_geom& g, const pbbss::MaskTargets& t, void* out,
                          int out_is_f64, int32_t* status, void* stream) {
  void* work = nullptr;
  const size_t bytes = pbbss::mask_threshold_work_bytes(g, t);
  if (bytes) {
    work = h->work.grow(bytes);
    if (!work) return PBBSS_ERR_HIP;
  }
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_mask_threshold(x, x_is_c128, g, t, work, out, out_is_f64, status,
                                      as_stream(stream));
}

PBBSS_API int pbbss_mask_lorenz(pbbss_handle_t h, const void* x, int x_is_c128,
                                const pbbss_mask_geom* geom, double lorenz_fraction,
                                double value_high, double value_low, void* out, int out_is_f64,
                                int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !geom || !out || !out_status) return PBBSS_ERR_INVALID_ARG;
  pbbss::MaskTargets t{};
  t.J = 1;
  t.lorenz = 1;
  t.fraction = lorenz_fraction;
  t.high = value_high;
  t.low = value_low;
  return mask_threshold(h, x, x_is_c128, *geom, t, out, out_is_f64, out_status, stream);
}

PBBSS_API int pbbss_mask_quantile(pbbss_handle_t h, const void* x, int x_is_c128,
                                  const pbbss_mask_geom* geom, int num_quantiles,
                                  const int64_t* lower_rank, const double* gamma,
                                  const int32_t* negative, double value_high, double value_low,
                                  void* out, int out_is_f64, int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !geom || !out || !out_status || !lower_rank || !gamma || !negative ||
      num_quantiles < 1)
    return PBBSS_ERR_INVALID_ARG;
  if (num_quantiles > pbbss::kMaskMaxQ) return PBBSS_ERR_UNSUPPORTED;
  if (geom->sensors != 1) return PBBSS_ERR_UNSUPPORTED;  // mask_module.py:443: no pooling rule
  pbbss::MaskTargets t{};
  t.J = num_quantiles;
  for (int j = 0; j < num_quantiles; ++j) {
    t.rank[j] = lower_rank[j];
    t.gamma[j] = gamma[j];
    t.negative[j] = negative[j] != 0;
  }
  t.high = value_high;
  t.low = value_low;
  return mask_threshold(h, x, x_is_c128, *geom, t, out, out_is_f64, out_status, stream);
}
