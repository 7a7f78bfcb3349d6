// extern "C" boundary of the cACGMM fits (include/pbbss.h; fused kernels: em_inst.hip,
// em32_inst.hip, shared_inst.hip; generic sizes: generic.hip): argument validation and the
// workspaces.  No device code lives here.
#include "handle.hpp"
#include "generic.hpp"

using pbbss::as_stream, pbbss::Carver, pbbss::carve, pbbss::DeviceGuard, pbbss::TimedRegion,
    pbbss::ResidencyGate;

// what the EmArgs of pbbss_cacgmm_fit and pbbss_cacgmm_fit_shared have in common; the class
// weights (strides and output) are the caller's
static pbbss::EmArgs cacgmm_em_args(const void* y, int64_t B, int T, const double* gamma0,
                                    const void* in_eigvec, const double* in_eigval,
                                    const double* in_weight, const double* saliency,
                                    const uint8_t* activity, const pbbss_em_opts* o,
                                    void* out_eigvec, double* out_eigval, int32_t* out_status,
                                    double* out_affiliation, double* out_quadratic_form) {
  pbbss::EmArgs a{};
  a.y = y;
  a.B = B;
  a.T = T;
  a.gamma0 = gamma0;
  a.in_eigvec = static_cast<const double*>(in_eigvec);
  a.in_eigval = in_eigval;
  a.in_weight = in_weight;
  a.saliency = saliency;
  a.activity = activity;
  a.out_eigvec = static_cast<double*>(out_eigvec);
  a.out_eigval = out_eigval;
  a.out_status = out_status;
  a.out_aff = out_affiliation;
  a.out_q = out_quadratic_form;
  a.iterations = o->iterations;
  a.covariance_norm = o->covariance_norm;
  a.weight_mode = o->weight_mode;
  a.layout = o->layout;
  a.final_predict = o->final_predict && (out_affiliation || out_quadratic_form);
  a.force_eig = o->force_eig;
  a.aff_eps = o->affiliation_eps;
  a.final_eps = 0.0;  // model.predict: affiliation_eps = 0 (cacgmm.py:73)
  a.eig_floor = o->eigenvalue_floor;
  return a;
}

PBBSS_API int pbbss_cacgmm_fit(pbbss_handle_t h, const void* y, int64_t B, int T, int D, int K,
                               const double* gamma0, const void* in_eigvec,
                               const double* in_eigval, const double* in_weight,
                               const double* saliency, const uint8_t* activity,
                               const pbbss_em_opts* o, void* out_eigvec, double* out_eigval,
                               double* out_weight, int32_t* out_status, double* out_affiliation,
                               double* out_quadratic_form, void* stream) {
  DeviceGuard device_guard(h);
  ResidencyGate residency_gate(h, as_stream(stream),
                               o && ResidencyGate::may_split(h, B, D, o->iterations));
  if (!h || !y || !o || B <= 0 || T <= 0) return PBBSS_ERR_INVALID_ARG;
  if (o->iterations <= 0) return PBBSS_ERR_INVALID_ARG;  // cacgmm.py:200
  const bool has_gamma = gamma0 != nullptr;
  const bool has_model = in_eigvec && in_eigval && in_weight;
  if (has_gamma == has_model) return PBBSS_ERR_INVALID_ARG;  // xor, cacgmm.py:190
  if (!out_eigvec || !out_eigval || !out_weight || !out_status) return PBBSS_ERR_INVALID_ARG;
  if (o->covariance_norm < 0 || o->covariance_norm > 2) return PBBSS_ERR_INVALID_ARG;
  if (o->weight_mode < 0 || o->weight_mode > 1) return PBBSS_ERR_INVALID_ARG;
  if (o->precision != PBBSS_PRECISION_F64 && o->precision != PBBSS_PRECISION_F32)
    return PBBSS_ERR_INVALID_ARG;
  if (o->precision == PBBSS_PRECISION_F32 && (D > 8 || K > 6)) return PBBSS_ERR_UNSUPPORTED;
  if (D > 8 || K > 6) {
    // generic-size path (generic.hip: run_gen_cacgmm_fit; also more than 6 classes at any D)
    if (!pbbss::gen_em_supported(D, K)) return PBBSS_ERR_UNSUPPORTED;
    if (o->layout != PBBSS_LAYOUT_TD) return PBBSS_ERR_UNSUPPORTED;
    const size_t nkt = (size_t)B * K * T;
    const size_t nmat = (size_t)B * K;
    const size_t ny = (size_t)B * T * D * (o->y_is_c128 ? 16 : 8);
    const bool transpose = B <= 65535;  // frame-contiguous copy for the E-steps of the loop
    pbbss::GenCacgmmWork w{};
    const int rc_work = carve(h->work, [&](Carver& wc) {
      w.aff = wc.take<double>(nkt);
      w.mw = wc.take<double>(nkt);
      w.cov = wc.take<double>(nmat * D * D * 2);
      w.inv = wc.take<double>(pbbss::gen_state_doubles((int64_t)nmat, D));
      w.inv_logdet = wc.take<double>(nmat);
      w.inv_ok = wc.take<int32_t>(nmat);
      w.zero_bin = wc.take<int32_t>((size_t)B);
      w.csum = wc.take<double>(nmat);
      w.yt = transpose ? wc.take<char>(ny) : nullptr;
    });
    if (rc_work != PBBSS_OK) return rc_work;
    const pbbss::GenCacgmmFit f{y, o->y_is_c128, B, T, D, K, gamma0, in_eigvec, in_eigval,
                                in_weight, saliency, activity, o->iterations, o->covariance_norm,
                                o->weight_mode, o->force_eig, o->final_predict,
                                o->affiliation_eps, o->eigenvalue_floor, out_eigvec, out_eigval,
                                out_weight, out_status, out_affiliation, out_quadratic_form};
    TimedRegion tr(h, as_stream(stream));
    return pbbss::run_gen_cacgmm_fit(f, w, h->cfg, as_stream(stream));
  }
  if (D < 2 || D > 8 || K < 1 || K > 6) return PBBSS_ERR_UNSUPPORTED;
  const bool f32 = o->precision == PBBSS_PRECISION_F32;
  if (f32 && (o->y_is_c128 || out_quadratic_form)) return PBBSS_ERR_UNSUPPORTED;
  pbbss::EmArgs a = cacgmm_em_args(y, B, T, gamma0, in_eigvec, in_eigval, in_weight, saliency,
                                   activity, o, out_eigvec, out_eigval, out_status,
                                   out_affiliation, out_quadratic_form);
  a.wb = K;
  a.wk = 1;
  a.wt = 0;
  a.out_weight = out_weight;
  a.prof = h->prof;
  // timing of the fused EM launch: events on the kernel dispatch itself (em_launch.hpp), the
  // duration of the EM kernel as a kernel trace sees it (the split kernel of a remainder bin runs
  // concurrently on the side stream and is shorter)
  pbbss::EmLaunchCfg cfg = h->cfg;
  if (h->timing) {
    const int slot = (int)(h->ring_seq++ % pbbss_handle_s::kTimingRing);
    cfg.ev_t0 = h->ring0[slot];
    cfg.ev_t1 = h->ring1[slot];
  }
  int rc;
  if (f32) {
    rc = pbbss::em32_launch(D, K, a, cfg, as_stream(stream));
    // a long utterance does not fit the LDS-resident packed kernel: say "unsupported", the
    // float64 kernel (which has an HBM-scratch variant) serves it
    if (rc == PBBSS_ERR_LDS_CAPACITY) rc = PBBSS_ERR_UNSUPPORTED;
  } else {
    rc = pbbss::em_launch(D, K, o->y_is_c128, a, cfg, as_stream(stream));
  }
  // a launch that was refused (capacity, shape) recorded no events: give its ring slot back, or
  // pbbss_kernel_ms_lagged would read an unrecorded / stale pair for it
  if (rc != PBBSS_OK && h->timing) --h->ring_seq;
  return rc;
}

PBBSS_API int pbbss_cacgmm_fit_shared(pbbss_handle_t h, const void* y, int64_t B, int T, int D,
                                      int K, int64_t group, const double* gamma0,
                                      const void* in_eigvec, const double* in_eigval,
                                      const double* in_weight, const double* saliency,
                                      const uint8_t* activity, const pbbss_em_opts* o,
                                      void* out_eigvec, double* out_eigval, double* out_weight,
                                      int32_t* out_status, double* out_affiliation,
                                      double* out_quadratic_form, void* stream) {
  DeviceGuard device_guard(h);
  ResidencyGate residency_gate(h, as_stream(stream));  // see ResidencyGate
  if (!h || !y || !o || B <= 0 || T <= 0 || group <= 0 || B % group != 0)
    return PBBSS_ERR_INVALID_ARG;
  if (o->iterations <= 0) return PBBSS_ERR_INVALID_ARG;  // cacgmm.py:200
  const bool has_gamma = gamma0 != nullptr;
  const bool has_model = in_eigvec && in_eigval && in_weight;
  if (has_gamma == has_model) return PBBSS_ERR_INVALID_ARG;  // xor, cacgmm.py:190
  if (!out_eigvec || !out_eigval || !out_weight || !out_status) return PBBSS_ERR_INVALID_ARG;
  if (o->covariance_norm < 0 || o->covariance_norm > 2) return PBBSS_ERR_INVALID_ARG;
  if (o->weight_mode != PBBSS_WEIGHT_SHARED_K && o->weight_mode != PBBSS_WEIGHT_SHARED_KT)
    return PBBSS_ERR_INVALID_ARG;
  if (D < 2 || D > 8 || K < 1 || K > 4 || group > INT32_MAX) return PBBSS_ERR_UNSUPPORTED;
  pbbss::EmArgs a = cacgmm_em_args(y, B, T, gamma0, in_eigvec, in_eigval, in_weight, saliency,
                                   activity, o, out_eigvec, out_eigval, out_status,
                                   out_affiliation, out_quadratic_form);
  a.wgroup = (int)group;
  a.out_weight_shared = out_weight;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::em_shared_launch(D, K, o->y_is_c128, a, h->cfg, as_stream(stream));
}

PBBSS_API int pbbss_cacgmm_predict(pbbss_handle_t h, const void* y, int64_t B, int T, int D,
                                   int K, const void* eigvec, const double* eigval,
                                   const double* weight, int64_t wb, int64_t wk, int64_t wt,
                                   const uint8_t* activity, int layout, int y_is_c128,
                                   double affiliation_eps, double* out_affiliation,
                                   double* out_quadratic_form, double* out_log_pdf,
                                   void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !eigvec || !eigval || !weight || B <= 0 || T <= 0) return PBBSS_ERR_INVALID_ARG;
  if (!out_affiliation && !out_quadratic_form && !out_log_pdf) return PBBSS_ERR_INVALID_ARG;
  if (D > 8 || K > 6) {
    if (!pbbss::gen_em_supported(D, K)) return PBBSS_ERR_UNSUPPORTED;
    const size_t ninv = pbbss::gen_state_doubles(B * K, D);
    double *inv, *inv_logdet;
    const int rc = carve(h->work, [&](Carver& wc) {
      inv = wc.take<double>(ninv);
      inv_logdet = wc.take<double>((size_t)B * K);
    });
    if (rc != PBBSS_OK) return rc;
    TimedRegion tr(h, as_stream(stream));
    pbbss::GenEstepArgs e{y, y_is_c128, layout, B, T, D, K, static_cast<const double*>(eigvec),
                          eigval, weight, wb, wk, wt};
    e.activity = activity;
    e.eps = affiliation_eps;
    e.out_aff = out_affiliation;
    e.out_q = out_quadratic_form;
    e.out_logpdf = out_log_pdf;
    return pbbss::launch_gen_estep(e, pbbss::GenInverseState{inv, inv_logdet, nullptr},
                                   as_stream(stream));
  }
  if (D < 2 || D > 8 || K < 1 || K > 6) return PBBSS_ERR_UNSUPPORTED;
  pbbss::EmArgs a{};
  a.y = y;
  a.B = B;
  a.T = T;
  a.in_eigvec = static_cast<const double*>(eigvec);
  a.in_eigval = eigval;
  a.in_weight = weight;
  a.wb = wb;
  a.wk = wk;
  a.wt = wt;
  a.final_activity = activity;  // CACGMM.predict(source_activity_mask=...)
  a.out_aff = out_affiliation;
  a.out_q = out_quadratic_form;
  a.out_logpdf = out_log_pdf;
  a.iterations = 0;
  a.layout = layout;
  a.final_predict = 1;
  a.final_eps = affiliation_eps;
  a.covariance_norm = PBBSS_COVNORM_EIGENVALUE;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::em_launch(D, K, y_is_c128, a, h->cfg, as_stream(stream));
}

PBBSS_API int pbbss_cacg_m_step(pbbss_handle_t h, const void* y, int64_t B, int T, int D, int K,
                                const double* saliency, const double* quadratic_form, int layout,
                                int y_is_c128, int covariance_norm, double eigenvalue_floor,
                                void* out_eigvec, double* out_eigval, void* out_cov,
                                int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !saliency || B <= 0 || T <= 0) return PBBSS_ERR_INVALID_ARG;
  if (!out_eigvec || !out_eigval || !out_status) return PBBSS_ERR_INVALID_ARG;
  if (covariance_norm < 0 || covariance_norm > 2) return PBBSS_ERR_INVALID_ARG;
  if (D > 8 || K > 6) {
    hipStream_t s = as_stream(stream);
    double* cov = static_cast<double*>(out_cov);
    if (!cov) {
      cov = static_cast<double*>(h->work.grow((size_t)B * K * D * D * 16));
      if (!cov) return PBBSS_ERR_HIP;
    }
    int rc = pbbss::launch_gen_cov(y, y_is_c128, layout, B, T, D, K, saliency, (int64_t)K * T,
                                   quadratic_form, nullptr, 0, PBBSS_WEIGHT_PER_CLASS_MEAN, cov,
                                   nullptr, nullptr, h->cfg.lds_limit, s);
    if (rc != PBBSS_OK) return rc;
    return pbbss::launch_gen_heev(cov, B * K, D, covariance_norm, eigenvalue_floor, out_eigval,
                                  static_cast<double*>(out_eigvec), out_status, h->cfg.lds_limit,
                                  s);
  }
  if (D < 2 || D > 8 || K < 1 || K > 6) return PBBSS_ERR_UNSUPPORTED;
  pbbss::EmArgs a{};
  a.y = y;
  a.B = B;
  a.T = T;
  a.gamma0 = saliency;         // the "masked affiliation" (cacgmm.py:332-338)
  a.q0 = quadratic_form;       // null = ones
  a.out_eigvec = static_cast<double*>(out_eigvec);
  a.out_eigval = out_eigval;
  a.out_status = out_status;
  a.out_cov = static_cast<double*>(out_cov);
  a.iterations = 1;
  a.covariance_norm = covariance_norm;
  a.weight_mode = PBBSS_WEIGHT_PER_CLASS_MEAN;
  a.layout = layout;
  a.eig_floor = eigenvalue_floor;
  return pbbss::em_launch(D, K, y_is_c128, a, h->cfg, as_stream(stream));
}
