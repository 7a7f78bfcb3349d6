// extern "C" boundary of the real-embedding mixtures (include/pbbss.h, N2; kernels: embed.hip,
// embed_wide.hip, vmf_bin.hip, mixw.hip, gauss_full.hip; EM loops: embed_fit.hip, gauss_full.hip):
// argument validation and the workspaces.  The joint spatial+spectral models: capi_joint.hip.
// No device code lives here.
#include "handle.hpp"
#include "gauss_full.hpp"
#include "generic.hpp"

using pbbss::as_stream, pbbss::embed_shape_ok, pbbss::Carver, pbbss::carve, pbbss::DeviceGuard,
    pbbss::TimedRegion;

PBBSS_API int pbbss_embed_log_pdf(pbbss_handle_t h, const void* y, int y_is_f64, int64_t B,
                                  int64_t N, int E, int K, int kind, const double* mean,
                                  const double* scale, double* out_log_pdf, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !mean || !scale || !out_log_pdf) return PBBSS_ERR_INVALID_ARG;
  if (!embed_shape_ok(B, N, E, K)) return PBBSS_ERR_UNSUPPORTED;
  hipStream_t s = as_stream(stream);
  if (K > pbbss::kEmbedMaxK) {  // class tiles on the matrix pipe (embed_wide.hip), no transposed copy
    void* w = h->work.grow(pbbss::embed_wide_work_doubles(B, N, E, K) * 8);
    if (!w) return PBBSS_ERR_HIP;
    return pbbss::embed_wide_log_pdf(kind, y, y_is_f64, B, N, E, K, mean, scale, 1.0, N,
                                     static_cast<double*>(w), out_log_pdf, h->cfg.lds_limit, s);
  }
  const size_t esz = y_is_f64 ? 8 : 4;
  char* yd;
  double *offset, *prec;
  int rc = carve(h->work, [&](Carver& wc) {
    yd = wc.take<char>((size_t)B * E * N * esz);
    offset = wc.take<double>((size_t)B * K);
    prec = wc.take<double>((size_t)B * K);
  });
  if (rc != PBBSS_OK) return rc;
  rc = pbbss::launch_embed_prepare(y, y_is_f64, B, N, E, 0, yd, nullptr, s);
  if (rc != PBBSS_OK) return rc;
  if (kind == PBBSS_EMBED_GAUSS_DIAG) {
    if (B != 1) return PBBSS_ERR_UNSUPPORTED;  // the reference's DiagonalGaussian has no batch axis
    void* cw = h->scratch.grow(pbbss::diag_consts_doubles(K, E) * 8);
    if (!cw) return PBBSS_ERR_HIP;
    return pbbss::launch_diag_estep(yd, y_is_f64, N, E, K, mean, scale, 1.0, N,
                                    static_cast<double*>(cw), out_log_pdf, s);
  }
  rc = pbbss::launch_embed_offsets(kind, B * K, E, scale, offset, prec, s);
  if (rc != PBBSS_OK) return rc;
  return pbbss::launch_embed_estep(kind, yd, y_is_f64, B, N, E, K, mean, prec, offset, nullptr,
                                   1.0, N, out_log_pdf, nullptr, s);
}

PBBSS_API int pbbss_estimate_mixture_weight(pbbss_handle_t h, const double* affiliation,
                                            const double* saliency, int64_t Bo, int64_t Bi, int K,
                                            int64_t N, int reduce_inner, int reduce_n,
                                            double* out_weight, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !affiliation || !out_weight || Bo <= 0 || Bi <= 0 || N <= 0) return PBBSS_ERR_INVALID_ARG;
  if (K < 1 || K > 64 || (saliency && K > 16)) return PBBSS_ERR_UNSUPPORTED;
  void* w = h->work.grow(pbbss::mixture_weight_tmp_doubles(Bo, Bi, K, N, reduce_n) * 8);
  if (!w) return PBBSS_ERR_HIP;
  return pbbss::launch_mixture_weight(affiliation, saliency, Bo, Bi, K, N, reduce_inner ? 1 : 0,
                                      reduce_n ? 1 : 0, static_cast<double*>(w), out_weight,
                                      as_stream(stream));
}

PBBSS_API int pbbss_log_pdf_to_affiliation(pbbss_handle_t h, const double* log_pdf, int64_t B, int K,
                                           int64_t N, const double* weight, int64_t wb, int64_t wk,
                                           int64_t wn, const uint8_t* activity,
                                           double affiliation_eps, double* out_affiliation,
                                           void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !log_pdf || !weight || !out_affiliation || B <= 0 || N <= 0 || K < 1)
    return PBBSS_ERR_INVALID_ARG;
  if (wb < 0 || wk < 0 || wn < 0) return PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_log_pdf_to_affiliation(log_pdf, B, K, N, weight, wb, wk, wn, activity,
                                              affiliation_eps, out_affiliation, as_stream(stream));
}

PBBSS_API int pbbss_log_pdf_to_affiliation_inline_pa(
    pbbss_handle_t h, const double* spatial_log_pdf, const double* spectral_log_pdf, int64_t F, int K,
    int64_t T, const double* weight, int64_t wb, int64_t wk, int64_t wn, const uint8_t* activity,
    double affiliation_eps, double* out_affiliation, int32_t* out_permutation, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !spatial_log_pdf || !spectral_log_pdf || !weight || !out_affiliation || F <= 0 ||
      T <= 0 || K < 1)
    return PBBSS_ERR_INVALID_ARG;
  if (wb < 0 || wk < 0 || wn < 0) return PBBSS_ERR_INVALID_ARG;
  if (T > 2147483647LL) return PBBSS_ERR_UNSUPPORTED;
  // the permutation search of the generic-size joint E-step without its M-step half: no
  // observation, no quadratic forms (K > 6: 5 040+ permutations per bin -- refused)
  return pbbss::launch_gen_joint_pa(nullptr, 0, F, (int)T, 0, K, spatial_log_pdf, nullptr,
                                    spectral_log_pdf, 1.0, weight, wb, wk, wn, nullptr,
                                    affiliation_eps, out_affiliation, nullptr, nullptr,
                                    as_stream(stream), activity, out_permutation);
}

PBBSS_API int pbbss_embed_fit(pbbss_handle_t h, const void* y, int y_is_f64, int64_t B, int64_t N,
                              int E, int K, int kind, int normalize, const double* weights,
                              double min_concentration, double max_concentration,
                              double* out_mean, double* out_scale, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !weights || !out_mean || !out_scale) return PBBSS_ERR_INVALID_ARG;
  if (!embed_shape_ok(B, N, E, K)) return PBBSS_ERR_UNSUPPORTED;
  hipStream_t s = as_stream(stream);
  if (K > pbbss::kEmbedMaxK) {
    void* w = h->work.grow(pbbss::embed_wide_work_doubles(B, N, E, K) * 8);
    if (!w) return PBBSS_ERR_HIP;
    return pbbss::embed_wide_fit(kind, y, y_is_f64, B, N, E, K, weights, normalize,
                                 min_concentration, max_concentration, static_cast<double*>(w),
                                 out_mean, out_scale, h->cfg.lds_limit, s);
  }
  const size_t np = pbbss::embed_partial_doubles(B, N, E, K, nullptr);
  double *part, *yd, *yn;
  int rc = carve(h->work, [&](Carver& wc) {
    part = wc.take<double>(np);
    yd = normalize ? wc.take<double>((size_t)B * N * E) : nullptr;
    yn = normalize ? wc.take<double>((size_t)B * N * E) : nullptr;
  });
  if (rc != PBBSS_OK) return rc;
  const void* yr = y;
  int yr_f64 = y_is_f64;
  if (normalize) {
    rc = pbbss::launch_embed_prepare(y, y_is_f64, B, N, E, 1, yd, yn, s);
    if (rc != PBBSS_OK) return rc;
    yr = yn;
    yr_f64 = 1;
  }
  return pbbss::launch_embed_fit(kind, yr, yr_f64, B, N, E, K, weights, N, nullptr,
                                 min_concentration, max_concentration, -1, part, out_mean,
                                 out_scale, nullptr, nullptr, nullptr, 0, s);
}

PBBSS_API int pbbss_gauss_full_fit(pbbss_handle_t h, const void* y, int y_is_f64, int64_t B,
                                   int64_t N, int E, int K, const double* weights,
                                   double* out_mean, double* out_covariance, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !weights || !out_mean || !out_covariance || B <= 0 || N <= 0)
    return PBBSS_ERR_INVALID_ARG;
  if (E < 1 || E > pbbss::kGaussFullMaxE || K < 1) return PBBSS_ERR_UNSUPPORTED;
  const size_t np = pbbss::gauss_full_partial_doubles(B, N, E, K);
  void* w = h->work.grow(np * 8);
  if (!w) return PBBSS_ERR_HIP;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_gauss_full_fit(y, y_is_f64, B, N, E, K, weights, nullptr,
                                      static_cast<double*>(w), out_mean, out_covariance, nullptr,
                                      nullptr, nullptr, nullptr, as_stream(stream));
}

PBBSS_API int pbbss_gauss_full_log_pdf(pbbss_handle_t h, const void* y, int y_is_f64, int64_t B,
                                       int64_t N, int E, int K, const double* mean,
                                       const double* covariance, double* out_log_pdf,
                                       int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !mean || !covariance || !out_log_pdf || !out_status || B <= 0 || N <= 0)
    return PBBSS_ERR_INVALID_ARG;
  if (E < 1 || E > pbbss::kGaussFullMaxE || K < 1 || K > 64) return PBBSS_ERR_UNSUPPORTED;
  const size_t nm = (size_t)B * K * E * E;
  double *mq, *off;
  int rc = carve(h->work, [&](Carver& wc) {
    mq = wc.take<double>(nm);
    off = wc.take<double>((size_t)B * K);
  });
  if (rc != PBBSS_OK) return rc;
  hipStream_t s = as_stream(stream);
  TimedRegion tr(h, s);
  rc = pbbss::launch_gauss_full_factor(covariance, B * K, E, mq, off, out_status, s);
  if (rc != PBBSS_OK) return rc;
  return pbbss::launch_gauss_full_logpdf(y, y_is_f64, B, N, E, K, mean, mq, off, nullptr,
                                         out_log_pdf, nullptr, s);
}

PBBSS_API int pbbss_gmm_full_fit(pbbss_handle_t h, const void* y, int64_t B, int64_t N, int E,
                                 int K, const double* gamma0, const double* in_mean,
                                 const double* in_covariance, const double* in_weight,
                                 const double* saliency, const double* fixed_covariance,
                                 const pbbss_mix_opts* o, double* out_mean,
                                 double* out_covariance, double* out_weight,
                                 double* out_affiliation, double* out_log_pdf,
                                 int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !o || !out_status || B <= 0 || N <= 0) return PBBSS_ERR_INVALID_ARG;
  if (E < 1 || E > pbbss::kGaussFullMaxE || K < 1 || K > 64) return PBBSS_ERR_UNSUPPORTED;
  if (o->iterations < 0 || o->weight_mode < 0 || o->weight_mode > 1) return PBBSS_ERR_INVALID_ARG;
  const bool has_gamma = gamma0 != nullptr;
  const bool has_model = in_mean && in_covariance && in_weight;
  if (has_gamma == has_model) return PBBSS_ERR_INVALID_ARG;
  if ((o->iterations == 0) != has_model) return PBBSS_ERR_INVALID_ARG;
  if (!out_mean || !out_covariance || !out_weight) return PBBSS_ERR_INVALID_ARG;
  pbbss::GmmFullWork w{};
  const int rc = carve(h->work, [&](Carver& wc) {
    w.part = wc.take<double>(pbbss::gauss_full_partial_doubles(B, N, E, K));
    w.mq = wc.take<double>((size_t)B * K * E * E);
    w.aff = wc.take<double>((size_t)B * K * N);
    w.off = wc.take<double>((size_t)B * K);
    w.s0 = wc.take<double>((size_t)B * K);
  });
  if (rc != PBBSS_OK) return rc;
  const pbbss::GmmFullFit f{y, o->embedding_is_f64, B, N, E, K, gamma0, in_mean, in_covariance,
                            in_weight, saliency, fixed_covariance, o->iterations, o->weight_mode,
                            o->final_predict, out_mean, out_covariance, out_weight,
                            out_affiliation, out_log_pdf, out_status};
  TimedRegion tr(h, as_stream(stream));
  return pbbss::run_gmm_full_fit(f, w, as_stream(stream));
}

// What pbbss_vmfmm_fit and pbbss_gmm_fit have in common: kind = PBBSS_EMBED_VMF or
// PBBSS_EMBED_GAUSS_SPHERICAL (fixed_scale = fixed_covariance (B,K) or null); the loop itself is
// run_embed_mixture_fit (embed_fit.hip).
static int embed_mixture_fit(pbbss_handle_t h, int kind, const void* y, int64_t B, int64_t N, int E,
                             int K, const double* gamma0, const double* in_mean,
                             const double* in_scale, const double* in_weight,
                             const double* saliency, const double* fixed_scale,
                             const pbbss_mix_opts* o, double* out_mean, double* out_scale,
                             double* out_weight, double* out_affiliation, double* out_log_pdf,
                             void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !o) return PBBSS_ERR_INVALID_ARG;
  if (!embed_shape_ok(B, N, E, K)) return PBBSS_ERR_UNSUPPORTED;
  if (o->iterations < 0 || o->weight_mode < 0 || o->weight_mode > 1) return PBBSS_ERR_INVALID_ARG;
  const bool has_gamma = gamma0 != nullptr;
  const bool has_model = in_mean && in_scale && in_weight;
  if (has_gamma == has_model) return PBBSS_ERR_INVALID_ARG;
  if ((o->iterations == 0) != has_model) return PBBSS_ERR_INVALID_ARG;  // vmfmm.py:70-74
  if (!out_mean || !out_scale || !out_weight) return PBBSS_ERR_INVALID_ARG;
  const pbbss::EmbedMixtureFit f{kind, y, o->embedding_is_f64, B, N, E, K, gamma0, in_mean,
                                 in_scale, in_weight, saliency, fixed_scale, o->iterations,
                                 o->weight_mode, o->final_predict, o->min_concentration,
                                 o->max_concentration, out_mean, out_scale, out_weight,
                                 out_affiliation, out_log_pdf};
  using Path = pbbss::EmbedFitPath;
  const Path path = pbbss::embed_mixture_path(f, h->cfg.lds_limit);
  const bool fused = path == Path::kFused;
  // the transposed copy: E-steps of the two-kernel path, and the log-pdf output of the fused one
  const bool need_copy = !fused || (o->final_predict && out_log_pdf);
  const size_t np = pbbss::embed_partial_doubles(B, N, E, K, nullptr);
  const size_t npf = fused ? pbbss::vmf_fused_partial_doubles(B, N, E, K, o->embedding_is_f64) : 0;
  pbbss::EmbedMixtureWork w{};
  int rc = PBBSS_OK;
  if (path == Path::kWide) {
    w.wide = static_cast<double*>(h->work.grow(pbbss::embed_wide_work_doubles(B, N, E, K) * 8));
    if (!w.wide) return PBBSS_ERR_HIP;
  } else if (path != Path::kPerBin) {  // (the per-mixture kernel keeps everything in LDS)
    rc = carve(h->work, [&](Carver& wc) {
      w.yd = need_copy ? wc.take<double>((size_t)B * N * E) : nullptr;
      w.rowscale = need_copy ? wc.take<double>((size_t)B * N) : nullptr;
      w.aff = fused ? nullptr : wc.take<double>((size_t)B * K * N);
      w.part = wc.take<double>(np > npf ? np : npf);
      w.offset = wc.take<double>((size_t)B * K);
      w.prec = wc.take<double>((size_t)B * K);
    });
  }
  if (rc != PBBSS_OK) return rc;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::run_embed_mixture_fit(path, f, w, h->cfg.lds_limit, h->cfg.num_cu,
                                      as_stream(stream));
}

PBBSS_API int pbbss_vmfmm_fit(pbbss_handle_t h, const void* y, int64_t B, int64_t N, int E, int K,
                              const double* gamma0, const double* in_mean,
                              const double* in_concentration, const double* in_weight,
                              const double* saliency, const pbbss_mix_opts* o, double* out_mean,
                              double* out_concentration, double* out_weight,
                              double* out_affiliation, double* out_log_pdf, void* stream) {
  return embed_mixture_fit(h, PBBSS_EMBED_VMF, y, B, N, E, K, gamma0, in_mean, in_concentration,
                           in_weight, saliency, nullptr, o, out_mean, out_concentration,
                           out_weight, out_affiliation, out_log_pdf, stream);
}

PBBSS_API int pbbss_gmm_fit(pbbss_handle_t h, const void* y, int64_t B, int64_t N, int E, int K,
                            const double* gamma0, const double* in_mean,
                            const double* in_covariance, const double* in_weight,
                            const double* saliency, const double* fixed_covariance,
                            const pbbss_mix_opts* o, double* out_mean, double* out_covariance,
                            double* out_weight, double* out_affiliation, double* out_log_pdf,
                            void* stream) {
  return embed_mixture_fit(h, PBBSS_EMBED_GAUSS_SPHERICAL, y, B, N, E, K, gamma0, in_mean,
                           in_covariance, in_weight, saliency, fixed_covariance, o, out_mean,
                           out_covariance, out_weight, out_affiliation, out_log_pdf, stream);
}
