// extern "C" boundary of the batched solvers and the beamformer family (include/pbbss.h; kernels:
// beamform.hip, bf_extra.hip, gev_general.hip, generic_bf.hip): argument validation and the choice
// between the D <= 8 and the generic-size kernels.  No device code lives here.
#include "handle.hpp"
#include "beamform.hpp"
#include "generic.hpp"
#include "generic_bf.hpp"

using pbbss::as_stream, pbbss::DeviceGuard;

PBBSS_API int pbbss_heev_batched(pbbss_handle_t h, const void* a, int64_t N, int D,
                                 double* out_eigval, void* out_eigvec, int32_t* out_status,
                                 void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !a || !out_eigval || !out_eigvec || N <= 0) return PBBSS_ERR_INVALID_ARG;
  if (D > 8)
    return pbbss::launch_gen_heev(static_cast<const double*>(a), N, D, -1, 0.0, out_eigval,
                                  static_cast<double*>(out_eigvec), out_status, h->cfg.lds_limit,
                                  as_stream(stream));
  return pbbss::launch_heev(static_cast<const double*>(a), N, D, out_eigval,
                            static_cast<double*>(out_eigvec), out_status, as_stream(stream));
}

PBBSS_API int pbbss_psd(pbbss_handle_t h, const void* x, int x_is_c128, int64_t B, int T, int D,
                        int K, const double* mask, int normalize, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !out || B <= 0 || T <= 0 || K <= 0) return PBBSS_ERR_INVALID_ARG;
  if (!mask && K != 1) return PBBSS_ERR_INVALID_ARG;
  if (D > 8 || K > 6) {
    return pbbss::launch_gen_cov(x, x_is_c128, PBBSS_LAYOUT_DT, B, T, D, K, mask, (int64_t)K * T,
                                 nullptr, nullptr, (mask && normalize) ? 1 : 2,
                                 PBBSS_WEIGHT_PER_CLASS_MEAN, static_cast<double*>(out), nullptr,
                                 nullptr, h->cfg.lds_limit, as_stream(stream));
  }
  return pbbss::launch_psd(x, x_is_c128, B, T, D, K, mask, normalize, static_cast<double*>(out),
                           h->cfg, as_stream(stream));
}

PBBSS_API int pbbss_gev(pbbss_handle_t h, const void* target, const void* noise, int64_t N,
                        int D, void* out_w, int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !target || !noise || !out_w || N <= 0) return PBBSS_ERR_INVALID_ARG;
  if (D > 8)
    return pbbss::launch_gen_gev(static_cast<const double*>(target),
                                 static_cast<const double*>(noise), N, D,
                                 static_cast<double*>(out_w), out_status, h->cfg.lds_limit,
                                 as_stream(stream));
  return pbbss::launch_gev(static_cast<const double*>(target), static_cast<const double*>(noise),
                           N, D, static_cast<double*>(out_w), out_status, as_stream(stream));
}

PBBSS_API int pbbss_gev_general(pbbss_handle_t h, const void* target, const void* noise,
                                int64_t N, int D, void* out_w, void* out_lambda,
                                int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !target || !noise || !out_w || N <= 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_gev_general(static_cast<const double*>(target),
                                   static_cast<const double*>(noise), N, D,
                                   static_cast<double*>(out_w), static_cast<double*>(out_lambda),
                                   out_status, as_stream(stream));
}

PBBSS_API int pbbss_solve(pbbss_handle_t h, const void* A, const void* Bm, int64_t N, int D,
                          int M, void* out_x, int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !A || !Bm || !out_x || N <= 0 || M <= 0) return PBBSS_ERR_INVALID_ARG;
  if (D > 8)
    return pbbss::launch_gen_solve(static_cast<const double*>(A), static_cast<const double*>(Bm),
                                   N, D, M, static_cast<double*>(out_x), out_status,
                                   h->cfg.lds_limit, as_stream(stream));
  if (M > 8) return PBBSS_ERR_UNSUPPORTED;
  return pbbss::launch_solve(static_cast<const double*>(A), static_cast<const double*>(Bm), N, D,
                             M, static_cast<double*>(out_x), out_status, as_stream(stream));
}

PBBSS_API int pbbss_mvdr_souden(pbbss_handle_t h, const void* target, const void* noise,
                                int64_t N, int D, double eps, void* out_mat, void* out_snr_num,
                                void* out_snr_den, int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !target || !noise || !out_mat || N <= 0) return PBBSS_ERR_INVALID_ARG;
  if (D > 8)
    return pbbss::launch_gen_souden(static_cast<const double*>(target),
                                    static_cast<const double*>(noise), N, D, eps, 0,
                                    static_cast<double*>(out_mat),
                                    static_cast<double*>(out_snr_num),
                                    static_cast<double*>(out_snr_den), out_status,
                                    h->cfg.lds_limit, as_stream(stream));
  return pbbss::launch_mvdr_souden(static_cast<const double*>(target),
                                   static_cast<const double*>(noise), N, D, eps, 0,
                                   static_cast<double*>(out_mat),
                                   static_cast<double*>(out_snr_num),
                                   static_cast<double*>(out_snr_den), out_status,
                                   as_stream(stream));
}

PBBSS_API int pbbss_mvdr(pbbss_handle_t h, const void* atf, const void* noise, int64_t N, int D,
                         void* out_w, int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !atf || !noise || !out_w || N <= 0) return PBBSS_ERR_INVALID_ARG;
  if (D > 8)
    return pbbss::launch_gen_mvdr(static_cast<const double*>(atf),
                                  static_cast<const double*>(noise), N, D,
                                  static_cast<double*>(out_w), out_status, h->cfg.lds_limit,
                                  as_stream(stream));
  return pbbss::launch_mvdr(static_cast<const double*>(atf), static_cast<const double*>(noise), N,
                            D, static_cast<double*>(out_w), out_status, as_stream(stream));
}

PBBSS_API int pbbss_ban(pbbss_handle_t h, const void* w, const void* noise, int64_t N, int D,
                        void* out_w, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !w || !noise || !out_w || N <= 0) return PBBSS_ERR_INVALID_ARG;
  if (D > 8)
    return pbbss::launch_gen_ban(static_cast<const double*>(w), static_cast<const double*>(noise),
                                 N, D, static_cast<double*>(out_w), as_stream(stream));
  return pbbss::launch_ban(static_cast<const double*>(w), static_cast<const double*>(noise), N, D,
                           static_cast<double*>(out_w), as_stream(stream));
}

PBBSS_API int pbbss_apply_beamforming_vector(pbbss_handle_t h, const void* w, const void* x,
                                             int x_is_c128, int64_t B, int T, int D, void* out,
                                             void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !w || !x || !out || B <= 0 || T <= 0 || D <= 0) return PBBSS_ERR_INVALID_ARG;
  if (D >= 30) return PBBSS_ERR_INVALID_ARG;  // beamformer.py:582
  for (int64_t b0 = 0; b0 < B; b0 += 65535) {
    int64_t nb = (B - b0 < 65535) ? (B - b0) : 65535;
    size_t esz = x_is_c128 ? 16 : 8;
    int rc = pbbss::launch_apply(static_cast<const double*>(w) + b0 * D * 2,
                                 (const char*)x + (size_t)b0 * D * T * esz, x_is_c128, nb, T, D,
                                 static_cast<double*>(out) + b0 * T * 2, as_stream(stream));
    if (rc != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}

PBBSS_API int pbbss_apply_beamforming_vector_shared(pbbss_handle_t h, const void* w, const void* x,
                                                    int x_is_c128, int64_t B, int64_t x_batch, int T,
                                                    int D, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !w || !x || !out || B <= 0 || T <= 0 || D <= 0 || x_batch <= 0 || B % x_batch != 0)
    return PBBSS_ERR_INVALID_ARG;
  if (D >= 30) return PBBSS_ERR_INVALID_ARG;  // beamformer.py:582
  for (int64_t b0 = 0; b0 < B; b0 += 65535) {
    int64_t nb = (B - b0 < 65535) ? (B - b0) : 65535;
    int rc = pbbss::launch_apply(static_cast<const double*>(w) + b0 * D * 2, x, x_is_c128, nb, T, D,
                                 static_cast<double*>(out) + b0 * T * 2, as_stream(stream), x_batch,
                                 b0);
    if (rc != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}

PBBSS_API int pbbss_select_reference_channel(pbbss_handle_t h, const void* mat, const void* snr_num,
                                             const void* snr_den, int64_t L, int64_t F, int D,
                                             int64_t lead_stride, int64_t bin_stride, double eps,
                                             void* out_w, int32_t* out_ref, int32_t* out_ok,
                                             void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !mat || !snr_num || !snr_den || !out_w || !out_ref || !out_ok || L <= 0 || F <= 0 ||
      D < 1 || lead_stride < 0 || bin_stride < 0 || out_w == mat)
    return PBBSS_ERR_INVALID_ARG;
  if (D > 32) return PBBSS_ERR_UNSUPPORTED;
  return pbbss::launch_select_reference_channel(
      static_cast<const double*>(mat), static_cast<const double*>(snr_num),
      static_cast<const double*>(snr_den), L, F, D, lead_stride, bin_stride, eps,
      static_cast<double*>(out_w), out_ref, out_ok, as_stream(stream));
}
PBBSS_API int pbbss_wmwf(pbbss_handle_t h, const void* target, const void* noise, int64_t N, int D,
                         double distortion_weight, int frequency_dependent, void* out_mat,
                         void* out_snr_num, void* out_snr_den, int32_t* out_status,
                         void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !target || !noise || !out_mat || N <= 0) return PBBSS_ERR_INVALID_ARG;
  if (D > 8)
    return pbbss::launch_gen_souden(static_cast<const double*>(target),
                                    static_cast<const double*>(noise), N, D, distortion_weight,
                                    frequency_dependent ? 2 : 1, static_cast<double*>(out_mat),
                                    static_cast<double*>(out_snr_num),
                                    static_cast<double*>(out_snr_den), out_status,
                                    h->cfg.lds_limit, as_stream(stream));
  return pbbss::launch_mvdr_souden(static_cast<const double*>(target),
                                   static_cast<const double*>(noise), N, D, distortion_weight,
                                   frequency_dependent ? 2 : 1, static_cast<double*>(out_mat),
                                   static_cast<double*>(out_snr_num),
                                   static_cast<double*>(out_snr_den), out_status,
                                   as_stream(stream));
}
PBBSS_API int pbbss_lcmv(pbbss_handle_t h, const void* atf, const void* response,
                         const void* noise, int64_t F, int D, int K, void* out_w,
                         int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !atf || !response || !noise || !out_w || F <= 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_lcmv(static_cast<const double*>(atf), static_cast<const double*>(response),
                            static_cast<const double*>(noise), F, D, K,
                            static_cast<double*>(out_w), out_status, as_stream(stream));
}

PBBSS_API int pbbss_phase_correction(pbbss_handle_t h, const void* vector, int64_t lead,
                                     int64_t rest, int F, int D, int two_d, void* scratch,
                                     void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !vector || !out || lead <= 0 || rest <= 0 || F <= 0 || D <= 0)
    return PBBSS_ERR_INVALID_ARG;
  if (F > 1 && !scratch) return PBBSS_ERR_INVALID_ARG;
  if (two_d && (lead != 1 || rest != 1)) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_phase_correction(static_cast<const double*>(vector), lead, rest, F, D,
                                        two_d, static_cast<double*>(scratch),
                                        static_cast<double*>(out), as_stream(stream));
}

PBBSS_API int pbbss_snr_postfilter(pbbss_handle_t h, const void* w, const void* target,
                                   const void* noise, int64_t F, int D, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !w || !target || !noise || !out || F <= 0 || D <= 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_bf_quadratic(0, static_cast<const double*>(w),
                                    static_cast<const double*>(target),
                                    static_cast<const double*>(noise), nullptr, F, D,
                                    static_cast<double*>(out), as_stream(stream));
}

PBBSS_API int pbbss_reference_channel_terms(pbbss_handle_t h, const void* w_mat, const void* target,
                                            const void* noise, int64_t F, int D, void* out_num,
                                            void* out_den, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !w_mat || !target || !noise || !out_num || !out_den || F <= 0 || D <= 0)
    return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_refch_terms(static_cast<const double*>(w_mat),
                                   static_cast<const double*>(target),
                                   static_cast<const double*>(noise), F, D,
                                   static_cast<double*>(out_num), static_cast<double*>(out_den),
                                   as_stream(stream));
}

PBBSS_API int pbbss_rank_one_approximation(pbbss_handle_t h, const void* covariance,
                                           const void* vector, int64_t N, int D, void* out,
                                           void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !covariance || !vector || !out || N <= 0 || D <= 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_rank_one(static_cast<const double*>(covariance),
                                static_cast<const double*>(vector), N, D,
                                static_cast<double*>(out), as_stream(stream));
}

PBBSS_API int pbbss_matvec(pbbss_handle_t h, const void* matrix, const void* vector, int64_t N,
                           int D, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !matrix || !vector || !out || N <= 0 || D <= 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_matvec(static_cast<const double*>(matrix),
                              static_cast<const double*>(vector), N, D, static_cast<double*>(out),
                              as_stream(stream));
}

PBBSS_API int pbbss_distortionless_normalization(pbbss_handle_t h, const void* w, const void* atf,
                                                 const void* noise, int64_t F, int D, void* out,
                                                 void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !w || !atf || !noise || !out || F <= 0 || D <= 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_bf_quadratic(1, static_cast<const double*>(w), nullptr,
                                    static_cast<const double*>(noise),
                                    static_cast<const double*>(atf), F, D,
                                    static_cast<double*>(out), as_stream(stream));
}

PBBSS_API int pbbss_zero_degree_normalization(pbbss_handle_t h, const void* vector, int64_t N,
                                              int D, int reference_channel, void* out,
                                              void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !vector || !out || N <= 0 || D <= 0) return PBBSS_ERR_INVALID_ARG;
  if (reference_channel < 0 || reference_channel >= D) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_zero_degree(static_cast<const double*>(vector), N, D, reference_channel,
                                   static_cast<double*>(out), as_stream(stream));
}

PBBSS_API int pbbss_condition_covariance(pbbss_handle_t h, const void* x, int64_t N, int D,
                                         double gamma, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !out || N <= 0 || D <= 0) return PBBSS_ERR_INVALID_ARG;
  // one thread per entry: the diagonal threads read the whole diagonal of x while their
  // neighbours store to out -- in place the trace would pick up conditioned entries
  if (x == out) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_condition_covariance(static_cast<const double*>(x), N, D, gamma,
                                            static_cast<double*>(out), as_stream(stream));
}

PBBSS_API int pbbss_apply_online_beamforming_vector(pbbss_handle_t h, const void* vector,
                                                    const void* mix, int mix_is_c128, int64_t F,
                                                    int T, int D, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !vector || !mix || !out || F <= 0 || T <= 0 || D <= 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_apply_online(static_cast<const double*>(vector), mix, mix_is_c128, F, T, D,
                                    static_cast<double*>(out), as_stream(stream));
}
