// extern "C" boundary of the directional mixtures, complex Watson and complex Bingham
// (include/pbbss.h; fused kernels: cw_inst.hip, cbmm_inst.hip; generic sizes: generic_watson.hip):
// argument validation and the workspaces.  No device code lives here.
#include "handle.hpp"
#include "generic.hpp"
#include "cbmm_launch.hpp"

using pbbss::as_stream, pbbss::Carver, pbbss::carve, pbbss::DeviceGuard, pbbss::TimedRegion,
    pbbss::ResidencyGate;

// the `.em` member the complex Watson and the complex Bingham fit have in common: per-bin class
// weights (K, 1, 0), (T, D) layout, log-pdf instead of quadratic forms as the second output
static pbbss::EmArgs directional_em_args(const void* y, int64_t B, int T, int K,
                                         const double* gamma0, const double* in_weight,
                                         const double* saliency, int iterations, int weight_mode,
                                         int final_predict, double* out_weight,
                                         int32_t* out_status, double* out_affiliation,
                                         double* out_log_pdf) {
  pbbss::EmArgs a{};
  a.y = y;
  a.B = B;
  a.T = T;
  a.gamma0 = gamma0;
  a.in_weight = in_weight;
  a.wb = K;
  a.wk = 1;
  a.wt = 0;
  a.saliency = saliency;
  a.out_weight = out_weight;
  a.out_status = out_status;
  a.out_aff = out_affiliation;
  a.out_logpdf = out_log_pdf;
  a.iterations = iterations;
  a.weight_mode = weight_mode;
  a.layout = PBBSS_LAYOUT_TD;
  a.final_predict = final_predict && (out_affiliation || out_log_pdf);
  return a;
}

PBBSS_API int pbbss_cwmm_fit(pbbss_handle_t h, const void* y, int64_t B, int T, int D, int K,
                             const double* gamma0, const void* in_mode,
                             const double* in_concentration, const double* in_weight,
                             const double* saliency, const pbbss_cwmm_opts* o,
                             const double* spline_t, const double* spline_c, void* out_mode,
                             double* out_concentration, double* out_weight, int32_t* out_status,
                             double* out_affiliation, double* out_log_pdf, void* stream) {
  DeviceGuard device_guard(h);
  // shared class weights run as ONE cooperative launch per batch of groups (cw_launch_shared)
  ResidencyGate residency_gate(
      h, as_stream(stream),
      o && (o->weight_mode == PBBSS_WEIGHT_SHARED_K || o->weight_mode == PBBSS_WEIGHT_SHARED_KT ||
            ResidencyGate::may_split(h, B, D, o->iterations)));
  if (!h || !y || !o || B <= 0 || T <= 0) return PBBSS_ERR_INVALID_ARG;
  if (o->iterations < 0) return PBBSS_ERR_INVALID_ARG;
  const bool has_gamma = gamma0 != nullptr;
  const bool has_model = in_mode && in_concentration && in_weight;
  if (has_gamma == has_model) return PBBSS_ERR_INVALID_ARG;
  if (o->iterations == 0 && !has_model) return PBBSS_ERR_INVALID_ARG;
  if (o->iterations > 0 && (!spline_t || !spline_c || o->n_coef < 3)) return PBBSS_ERR_INVALID_ARG;
  if (o->iterations > 0 && (!out_mode || !out_concentration || !out_weight))
    return PBBSS_ERR_INVALID_ARG;
  // PBBSS_WEIGHT_SHARED_K (round 4): weights averaged over groups of `opts->group` consecutive
  // problems (the bins of an utterance), fused kernels only, fit from affiliations only
  const bool shared_k = o->weight_mode == PBBSS_WEIGHT_SHARED_K ||
                        o->weight_mode == PBBSS_WEIGHT_SHARED_KT;  // (group, K) / (group, K, T)
  if (o->weight_mode < 0 || (o->weight_mode > 1 && !shared_k)) return PBBSS_ERR_INVALID_ARG;
  if (shared_k && (o->group < 1 || B % o->group != 0 || !has_gamma || o->iterations < 1))
    return PBBSS_ERR_INVALID_ARG;
  if (shared_k && (D > 8 || K > 4)) return PBBSS_ERR_UNSUPPORTED;
  if (D > 8 || K > 4) {
    // generic-size path (generic_watson.hip: run_gen_watson_fit); a model the caller does not
    // ask for lives in the work area
    if (!pbbss::gen_supported(D, K) || B > 65535) return PBBSS_ERR_UNSUPPORTED;
    const size_t nkt = (size_t)B * K * T, nmat = (size_t)B * K;
    pbbss::GenWatsonWork w{};
    double *mode_w, *conc_w, *weight_w;
    int32_t* status_w;
    const int rc = carve(h->work, [&](Carver& wc) {
      w.aff = wc.take<double>(nkt);
      w.lp = wc.take<double>(nkt);
      w.cov = wc.take<double>(nmat * D * D * 2);
      w.evec = wc.take<double>(nmat * D * D * 2);
      w.eval = wc.take<double>(nmat * D);
      mode_w = wc.take<double>(nmat * D * 2);
      conc_w = wc.take<double>(nmat);
      weight_w = wc.take<double>(nmat);
      w.lognorm = wc.take<double>(nmat);
      status_w = wc.take<int32_t>(nmat);
    });
    if (rc != PBBSS_OK) return rc;
    const pbbss::GenWatsonFit f{
        y, o->y_is_c128, B, T, D, K, gamma0, in_mode, in_concentration, in_weight, saliency,
        o->iterations, o->weight_mode, o->final_predict,
        {spline_t, spline_c, o->n_coef, o->ev_min, o->ev_max, o->max_concentration},
        out_mode ? static_cast<double*>(out_mode) : mode_w,
        out_concentration ? out_concentration : conc_w, out_weight ? out_weight : weight_w,
        out_status ? out_status : status_w, out_affiliation, out_log_pdf};
    TimedRegion tr(h, as_stream(stream));
    return pbbss::run_gen_watson_fit(f, w, h->cfg.lds_limit, as_stream(stream));
  }
  if (D < 2 || D > 8 || K < 1 || K > 4) return PBBSS_ERR_UNSUPPORTED;
  pbbss::WatsonArgs wa{};
  wa.em = directional_em_args(y, B, T, K, gamma0, in_weight, saliency, o->iterations,
                              o->weight_mode, o->final_predict, out_weight, out_status,
                              out_affiliation, out_log_pdf);
  if (shared_k) {  // out_weight is (B / group, K)
    wa.em.wgroup = o->group;
    wa.em.out_weight = nullptr;
    wa.em.out_weight_shared = out_weight;
  }
  wa.in_mode = static_cast<const double*>(in_mode);
  wa.in_conc = in_concentration;
  wa.spline_t = spline_t;
  wa.spline_c = spline_c;
  wa.n_coef = o->n_coef;
  wa.ev_min = o->ev_min;
  wa.ev_max = o->ev_max;
  wa.max_concentration = o->max_concentration;
  wa.out_mode = static_cast<double*>(out_mode);
  wa.out_conc = out_concentration;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::cw_launch(D, K, o->y_is_c128, wa, h->cfg, as_stream(stream));
}

PBBSS_API int pbbss_cbmm_fit(pbbss_handle_t h, const void* y, int64_t B, int T, int D, int K,
                             const double* gamma0, const void* in_eigvec, const double* in_eigval,
                             const double* in_weight, const double* saliency,
                             const pbbss_cbmm_opts* o, void* out_eigvec, double* out_eigval,
                             double* out_lognorm, double* out_weight, int32_t* out_status,
                             double* out_affiliation, double* out_log_pdf, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !o || B <= 0 || T <= 0) return PBBSS_ERR_INVALID_ARG;
  if (o->iterations < 0) return PBBSS_ERR_INVALID_ARG;
  const bool has_gamma = gamma0 != nullptr;
  const bool has_model = in_eigvec && in_eigval && in_weight;
  if (has_gamma == has_model) return PBBSS_ERR_INVALID_ARG;
  if (o->iterations == 0 && !has_model) return PBBSS_ERR_INVALID_ARG;
  if (o->iterations > 0 && (!out_eigvec || !out_eigval || !out_weight))
    return PBBSS_ERR_INVALID_ARG;
  if (o->weight_mode != PBBSS_WEIGHT_PER_CLASS_MEAN && o->weight_mode != PBBSS_WEIGHT_UNIFORM)
    return PBBSS_ERR_INVALID_ARG;
  if (!(o->max_concentration > 0.0) || !(o->eigenvalue_eps >= 0.0) || !(o->norm_eps >= 0.0))
    return PBBSS_ERR_INVALID_ARG;
  if (D < 2 || D > 8 || K < 1 || K > 4) return PBBSS_ERR_UNSUPPORTED;
  pbbss::BinghamArgs ba{};
  ba.em = directional_em_args(y, B, T, K, gamma0, in_weight, saliency, o->iterations,
                              o->weight_mode, o->final_predict, out_weight, out_status,
                              out_affiliation, out_log_pdf);
  ba.in_eigvec = static_cast<const double*>(in_eigvec);
  ba.in_eigval = in_eigval;
  ba.max_concentration = o->max_concentration;
  ba.eigenvalue_eps = o->eigenvalue_eps;
  ba.norm_eps = o->norm_eps;
  ba.out_eigvec = static_cast<double*>(out_eigvec);
  ba.out_eigval = out_eigval;
  ba.out_lognorm = out_lognorm;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::cb_launch(D, K, o->y_is_c128, ba, h->cfg, as_stream(stream));
}

PBBSS_API int pbbss_cbingham_find_eigenvalues(pbbss_handle_t h, const double* scatter_eigenvalues,
                                              int64_t N, int D, double eigenvalue_eps,
                                              double max_concentration, double* out_eigenvalues,
                                              int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !scatter_eigenvalues || !out_eigenvalues || !out_status || N <= 0)
    return PBBSS_ERR_INVALID_ARG;
  if (!(max_concentration > 0.0) || !(eigenvalue_eps >= 0.0)) return PBBSS_ERR_INVALID_ARG;
  if (D < 2 || D > 8) return PBBSS_ERR_UNSUPPORTED;
  return pbbss::cb_solve_launch(D, scatter_eigenvalues, N, eigenvalue_eps, max_concentration,
                                out_eigenvalues, out_status, h->cfg.num_cu, as_stream(stream));
}
