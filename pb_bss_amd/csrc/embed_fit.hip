// The EM loop of the two real-embedding mixtures (pbbss_vmfmm_fit / pbbss_gmm_fit) over the
// launchers of embed.hip, embed_wide.hip and vmf_bin.hip: a multi-kernel loop enqueued
// asynchronously on the stream (no host sync).  Host code only.
#include "embed.hpp"
#include "embed_wide.hpp"
#include "launch_util.hpp"

namespace pbbss {

EmbedFitPath embed_mixture_path(const EmbedMixtureFit& f, size_t lds_limit) {
  if (f.K > kEmbedMaxK) return EmbedFitPath::kWide;
  const bool vmf = f.kind == PBBSS_EMBED_VMF;
  // many small vMF mixtures (e.g. one per frequency bin): the persistent one-workgroup-per-mixture
  // kernel runs the whole loop in ONE launch; a big mixture is better off spread over the chip by
  // the sweep + finalize pairs of the other two paths
  if (vmf && !f.out_log_pdf && f.B >= 16) {
    const size_t lds = vmf_bin_lds_bytes(f.N, f.E, f.K, f.y_is_f64);
    if (lds > 0 && lds <= lds_limit) return EmbedFitPath::kPerBin;
  }
  // vMF mixture: one pass per iteration where the LDS tile fits; the two-kernel path otherwise,
  // for the Gaussian mixture and (its final E-step) for the log-pdf output
  const bool fused = vmf && vmf_fused_partial_doubles(f.B, f.N, f.E, f.K, f.y_is_f64) > 0;
  return fused ? EmbedFitPath::kFused : EmbedFitPath::kTwoKernel;
}

int run_embed_mixture_fit(EmbedFitPath path, const EmbedMixtureFit& f, const EmbedMixtureWork& w,
                          size_t lds_limit, int num_cu, hipStream_t s) {
  const int64_t B = f.B, N = f.N;
  const int E = f.E, K = f.K, kind = f.kind, e_f64 = f.y_is_f64;
  const bool vmf = kind == PBBSS_EMBED_VMF;
  const bool has_model = f.gamma0 == nullptr;
  const bool fused = path == EmbedFitPath::kFused;
  int rc;
  // Two-kernel path: the E-step reads the transposed copy, the M-step the caller's row-major
  // array, both in the caller's type.  The vMF mixture works on unit rows: the E-step normalises
  // its dot products itself, the M-step takes 1 / |y_n| from `rowscale`.
  if (w.yd) {
    rc = launch_embed_prepare(f.y, e_f64, B, N, E, 0, w.yd, nullptr, s, vmf ? w.rowscale : nullptr);
    if (rc != PBBSS_OK) return rc;
  }
  if (has_model) {
    rc = copy_model({f.out_mean, f.in_mean, (size_t)B * K * E * 8},
                    {f.out_scale, f.in_scale, (size_t)B * K * 8},
                    {f.out_weight, f.in_weight, (size_t)B * K * 8}, s);
    if (rc != PBBSS_OK) return rc;
  }
  if (path == EmbedFitPath::kWide)
    return embed_wide_mixture(kind, f.y, e_f64, B, N, E, K, f.gamma0, f.saliency, f.fixed_scale,
                              f.iterations, f.weight_mode, f.min_concentration,
                              f.max_concentration, w.wide, f.out_mean, f.out_scale, f.out_weight,
                              f.final_predict ? f.out_affiliation : nullptr,
                              f.final_predict ? f.out_log_pdf : nullptr, lds_limit, s);
  if (path == EmbedFitPath::kPerBin) {
    const double* m = has_model ? f.out_mean : nullptr;
    const double* c = has_model ? f.out_scale : nullptr;
    const double* wt = has_model ? f.out_weight : nullptr;
    double* out_aff = f.final_predict ? f.out_affiliation : nullptr;
    rc = launch_vmf_bin_em2(f.y, e_f64, B, N, E, K, f.iterations, f.gamma0, f.saliency, m, c, wt,
                            f.min_concentration, f.max_concentration, f.weight_mode, f.out_mean,
                            f.out_scale, f.out_weight, out_aff, lds_limit,
                            num_cu > 0 ? num_cu : 256, s);
    if (rc != PBBSS_ERR_UNSUPPORTED) return rc;
    return launch_vmf_bin_em(f.y, e_f64, B, N, E, K, f.iterations, f.gamma0, f.saliency, m, c, wt,
                             f.min_concentration, f.max_concentration, f.weight_mode, f.out_mean,
                             f.out_scale, f.out_weight, out_aff, lds_limit, s);
  }
  for (int it = 0; it < f.iterations; ++it) {
    if (fused) {  // vmfmm.py:131-172: E-step with the previous model (or the initialisation), M-step
      rc = launch_vmf_em(f.y, e_f64, B, N, E, K, it == 0 ? f.gamma0 : nullptr, f.saliency,
                         f.min_concentration, f.max_concentration, f.weight_mode, w.part,
                         f.out_mean, f.out_scale, f.out_weight, w.offset, w.prec, nullptr, 1, s);
      if (rc != PBBSS_OK) return rc;
      continue;
    }
    const double* src = f.gamma0;
    if (it > 0) {  // vmfmm.py:137-138 / gmm.py:129-130 (offsets: previous M-step's finalize)
      rc = launch_embed_estep(kind, w.yd, e_f64, B, N, E, K, f.out_mean, w.prec, w.offset,
                              f.out_weight, 1.0, N, nullptr, w.aff, s);
      if (rc != PBBSS_OK) return rc;
      src = w.aff;
    }
    rc = launch_embed_fit(kind, f.y, e_f64, B, N, E, K, src, N, f.saliency, f.min_concentration,
                          f.max_concentration, f.weight_mode, w.part, f.out_mean, f.out_scale,
                          f.out_weight, w.offset, w.prec, 0, s, vmf ? w.rowscale : nullptr);
    if (rc != PBBSS_OK) return rc;
    if (f.fixed_scale) {  // gmm.py:160-167
      if ((rc = copy_d2d(f.out_scale, f.fixed_scale, (size_t)B * K * 8, s)) != PBBSS_OK) return rc;
      rc = launch_embed_offsets(kind, B * K, E, f.out_scale, w.offset, w.prec, s);
      if (rc != PBBSS_OK) return rc;
    }
  }
  if (f.final_predict && (f.out_affiliation || f.out_log_pdf)) {
    if (f.iterations == 0) {
      rc = launch_embed_offsets(kind, B * K, E, f.out_scale, w.offset, w.prec, s);
      if (rc != PBBSS_OK) return rc;
    }
    if (fused && !f.out_log_pdf)
      return launch_vmf_em(f.y, e_f64, B, N, E, K, nullptr, nullptr, f.min_concentration,
                           f.max_concentration, f.weight_mode, w.part, f.out_mean, f.out_scale,
                           f.out_weight, w.offset, w.prec, f.out_affiliation, 0, s);
    return launch_embed_estep(kind, w.yd, e_f64, B, N, E, K, f.out_mean, w.prec, w.offset,
                              f.out_weight, 1.0, N, f.out_log_pdf, f.out_affiliation, s);
  }
  return PBBSS_OK;
}

}  // namespace pbbss
