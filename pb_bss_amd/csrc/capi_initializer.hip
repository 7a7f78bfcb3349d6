// extern "C" boundary of the deflation seed (include/pbbss.h; kernels: initializer.hip): argument
// validation and the workspace.  No device code lives here.
#include "handle.hpp"
#include "initializer.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

PBBSS_API int pbbss_deflation_seed(pbbss_handle_t h, const void* y, int y_is_c128, int64_t B, int F,
                                   int T, int D, int K, const double* saliency,
                                   int permutation_free, int neighbors, double eps,
                                   int round_begin, int round_end, int finalize,
                                   double* saliency_state, double* out_posterior,
                                   int32_t* out_peak, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !out_posterior || B <= 0 || F <= 0 || T <= 0) return PBBSS_ERR_INVALID_ARG;
  if (neighbors < 0 || T <= 2 * neighbors) return PBBSS_ERR_INVALID_ARG;
  if (D < 2 || D > 32 || K < 2 || K > 19) return PBBSS_ERR_UNSUPPORTED;
  if (round_begin < 0 || round_end < round_begin || round_end > K - 1) return PBBSS_ERR_INVALID_ARG;
  if (finalize && round_end != K - 1) return PBBSS_ERR_INVALID_ARG;
  // a call that continues, or is to be continued, needs the caller's state array
  const bool whole = round_begin == 0 && round_end == K - 1 && finalize;
  if (!whole && !saliency_state) return PBBSS_ERR_INVALID_ARG;
  pbbss::DeflationArgs a{};
  a.y = y;
  a.y_is_c128 = y_is_c128;
  a.B = B;
  a.F = F;
  a.T = T;
  a.D = D;
  a.K = K;
  a.sal_in = saliency;
  a.sal_state = saliency_state;
  a.permutation_free = permutation_free != 0;
  a.neighbors = neighbors;
  a.eps = eps;
  a.r0 = round_begin;
  a.r1 = round_end;
  a.finalize = finalize != 0;
  a.out = out_posterior;
  a.out_peak = out_peak;
  const int init = round_begin == 0;
  const size_t bytes = pbbss::deflation_work_bytes(a, init, h->cfg.lds_limit);
  void* work = nullptr;
  if (bytes) {
    work = h->work.grow(bytes);
    if (!work) return PBBSS_ERR_HIP;
  }
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_deflation_seed(a, init, work, h->cfg.lds_limit, as_stream(stream));
}
