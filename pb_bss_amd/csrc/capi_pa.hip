// extern "C" boundary of permutation alignment (include/pbbss.h; kernels: dhtv.hip): argument
// validation.  No device code lives here.
#include "handle.hpp"
#include "dhtv.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::ResidencyGate;

PBBSS_API int pbbss_dhtv_calculate_mapping(pbbss_handle_t h, const double* mask, int64_t U, int K,
                                           int F, int T, const int32_t* plan, int P, int optimal,
                                           int metric, double* scratch, int32_t* out_mapping,
                                           int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  ResidencyGate residency_gate(h, as_stream(stream));  // see ResidencyGate
  if (!h || !mask || !plan || !scratch || !out_mapping || !out_status) return PBBSS_ERR_INVALID_ARG;
  if (U <= 0 || F <= 0 || T <= 0 || P <= 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_dhtv(mask, U, K, F, T, plan, P, optimal, metric, scratch, out_mapping, out_status,
                            h->cfg.lds_limit, h->cfg.num_cu, h->dhtv_team, h->team_buf,
                            h->team_bytes, h->dhtv_probe, h->cfg.spin_limit, as_stream(stream));
}

PBBSS_API int pbbss_pa_pairwise_mapping(pbbss_handle_t h, const double* mask,
                                        const double* reference, int64_t U, int K, int64_t F,
                                        int T, const int64_t* mask_strides,
                                        const int64_t* reference_strides, int metric, int optimal,
                                        double* out_scores, int32_t* out_mapping, int64_t map_F,
                                        int64_t map_col0, int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !mask || !reference || !mask_strides || !reference_strides || !out_mapping ||
      !out_status)
    return PBBSS_ERR_INVALID_ARG;
  if (U <= 0 || F <= 0 || T <= 0 || map_col0 < 0 || map_col0 + F > map_F)
    return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_pa_pair(mask, reference, U, K, F, T, mask_strides, reference_strides,
                               metric, optimal, out_scores, out_mapping, map_F, map_col0,
                               out_status, as_stream(stream));
}

PBBSS_API int pbbss_pa_compose_mapping(pbbss_handle_t h, int32_t* mapping, int64_t U, int K,
                                       int64_t F, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !mapping || U <= 0 || F <= 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_pa_compose(mapping, U, K, F, as_stream(stream));
}

PBBSS_API int pbbss_pa_mapping_from_scores(pbbss_handle_t h, const double* scores, int64_t N,
                                           int K, int optimal, int32_t* out_mapping,
                                           int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !scores || !out_mapping || !out_status || N <= 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_pa_assign(scores, N, K, optimal, out_mapping, out_status,
                                 as_stream(stream));
}

PBBSS_API int pbbss_apply_mapping(pbbss_handle_t h, const double* mask, const int32_t* mapping,
                                  int64_t U, int K, int F, int T, double* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !mask || !mapping || !out || U <= 0 || K <= 0 || F <= 0 || T <= 0)
    return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_apply_mapping(mask, mapping, U, K, F, T, out, as_stream(stream));
}
