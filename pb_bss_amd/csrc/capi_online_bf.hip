// extern "C" boundary of the frame-recursive MVDR beamformer (include/pbbss.h, XIV; kernel:
// online_bf.hip): argument validation and the launch.  No device code lives here.
#include "handle.hpp"
#include "online_bf.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

PBBSS_API int pbbss_online_mvdr(pbbss_handle_t h, const void* y, int y_is_c128, int64_t B, int D,
                                int64_t T, int64_t stride_b, int64_t stride_d, int64_t stride_t,
                                const void* target_mask, const void* noise_mask, int mask_is_f64,
                                double alpha, int ref_channel, void* target_psd, void* noise_inv,
                                int64_t* frames_seen, void* out_x, void* out_w,
                                int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !target_mask || !noise_mask || !target_psd || !noise_inv || !frames_seen ||
      !out_x || !out_status || B < 1 || D < 1 || T < 1 || !(alpha > 0.0 && alpha <= 1.0) ||
      ref_channel < 0 || ref_channel >= D)
    return PBBSS_ERR_INVALID_ARG;
  if (D > pbbss::kOnlineBfMaxD || T > INT32_MAX / 4 || B > INT32_MAX) return PBBSS_ERR_UNSUPPORTED;
  TimedRegion tr(h, as_stream(stream));
  const pbbss::WpeFrames frames{y, y_is_c128, T, stride_b, stride_d, stride_t, D};
  const pbbss::OnlineBfArgs a{target_mask, noise_mask, mask_is_f64, alpha, ref_channel,
                              static_cast<double*>(target_psd), static_cast<double*>(noise_inv),
                              frames_seen, out_x, static_cast<double*>(out_w), out_status};
  return pbbss::launch_online_mvdr(frames, B, a, as_stream(stream));
}
