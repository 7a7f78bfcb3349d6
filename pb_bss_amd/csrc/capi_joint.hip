// extern "C" boundary of the joint spatial+spectral models (include/pbbss.h, N3): pbbss_joint_fit.
// The one entry point of the C-ABI layer that talks to the communicator, the side stream, the
// exchange buffer and four kernel families at once; a multi-kernel loop enqueued asynchronously on
// `stream` (no host sync).  No device code lives here.
#include "handle.hpp"
#include <cstdlib>
#include "gauss_full.hpp"
#include "generic.hpp"
#include "comm.hpp"

using pbbss::as_stream, pbbss::copy_d2d, pbbss::embed_shape_ok, pbbss::Carver, pbbss::carve,
    pbbss::DeviceGuard, pbbss::TimedRegion;

// dynamic LDS of the joint kernels for (D, K, T): the EM kernel's own figure + the 64 bytes of the
// inline aligner's class permutation.  0 outside the compiled range (D = 2..8, K = 1..6): those
// shapes are refused or take the generic-size path whatever the figure.
static size_t joint_lds_bytes(int D, int K, int T, int c128) {
  size_t lds = 0;
  (void)pbbss::dispatch_range<2, 8>(D, [&](auto d) {
    return pbbss::dispatch_range<1, 6>(K, [&](auto k) {
      return pbbss::dispatch_real(c128, [&](auto ys) {
        lds = pbbss::EmKernel<d(), k(), decltype(ys), false>::lds_bytes(T) + 64;
        return PBBSS_OK;
      });
    });
  });
  return lds;
}

// helper blocks of the in-launch spectral finalize of the rotated joint loop (embed_dev.hpp)
static constexpr int kJointFinHelpers = 32;
static int joint_fin_helpers() {  // development knob: helper blocks actually launched (<= 32)
  static const int n = [] {
    const char* v = getenv("PBBSS_JOINT_FIN_HELPERS");
    const int x = v ? atoi(v) : kJointFinHelpers;
    return x < 1 ? 1 : (x > kJointFinHelpers ? kJointFinHelpers : x);
  }();
  return n;
}

PBBSS_API int pbbss_joint_fit(pbbss_handle_t h, const void* observation, const void* embedding,
                              int64_t F, int T, int D, int E, int K, const double* gamma0,
                              const void* in_eigvec, const double* in_eigval,
                              const double* in_weight, const double* in_mean,
                              const double* in_scale, const double* saliency,
                              const pbbss_mix_opts* o, void* out_eigvec, double* out_eigval,
                              double* out_weight, double* out_mean, double* out_scale,
                              int32_t* out_status, double* out_affiliation, void* stream) {
  DeviceGuard device_guard(h);
  // (no residency gate: the member workgroups of the joint kernels never wait for each other --
  // the last arriver finishes the problem, run_joint_member in cacgmm_em.hpp)
  if (!h || !observation || !embedding || !o || F <= 0 || T <= 0) return PBBSS_ERR_INVALID_ARG;
  // 9 <= D <= 32 or 7..19 classes: the spatial half runs on the generic-size kernels
  // (generic.hip), one E-step and one M-step launch group per iteration around the same spectral
  // kernels (more than eight classes: the class-tile kernels of embed_wide.hip)
  // ... and so does an utterance too long for the LDS-resident joint kernels (no HBM-scratch
  // variant of those): the generic kernels stream the frames (round 4; the reference has no
  // length limit)
  const size_t joint_lds = joint_lds_bytes(D, K, T, o->obs_is_c128);
  const bool gen = D > 8 || K > 6 || joint_lds > h->cfg.lds_limit;
  if (D < 2 || K < 1 || (gen && !pbbss::gen_supported(D, K))) return PBBSS_ERR_UNSUPPORTED;
  const bool wide = K > pbbss::kEmbedMaxK;  // (K > 6 is always gen: K <= 19 by gen_supported)
  if (gen && (F > 65535 || (o->inline_pa && K > 6))) return PBBSS_ERR_UNSUPPORTED;
  const int64_t N = F * (int64_t)T;
  if (!embed_shape_ok(1, N, E, K)) return PBBSS_ERR_UNSUPPORTED;
  if (o->iterations < 0 || o->weight_mode < 0 || o->weight_mode > 4) return PBBSS_ERR_INVALID_ARG;
  if (o->kind < PBBSS_EMBED_VMF || o->kind > PBBSS_EMBED_GAUSS_DIAG) return PBBSS_ERR_UNSUPPORTED;
  const bool g_full = o->kind == PBBSS_EMBED_GAUSS_FULL, g_diag = o->kind == PBBSS_EMBED_GAUSS_DIAG;
  if (g_full && E > pbbss::kGaussFullMaxE) return PBBSS_ERR_UNSUPPORTED;
  // opts->sharded: this call holds ONE RANK'S BLOCK of the frequency bins; the spectral M-step
  // sums and the bin-constant class weights are summed over the communicator of the handle, in
  // stream order (no host round trip inside the loop).  The full-covariance scatter centres its
  // augmented vectors on a shift that must be THE SAME on every rank for the Gram tiles to add up:
  // rank 0's first embedding row, broadcast once per fit by an all-reduce (the others contribute
  // zeros); the reduced tiles are all-reduced between the reduction and the finalize kernel.
  const bool sharded = o->sharded != 0 && o->iterations > 0;
  // the class-tile fit takes its moments about the FIRST ROW OF THE RANK'S OWN block: partials of
  // different ranks do not add up -- sharded fits stay at K <= 8
  if (sharded && wide) return PBBSS_ERR_UNSUPPORTED;
  if (sharded && !h->comm) return PBBSS_ERR_INVALID_ARG;  // pbbss_comm_create first
  pbbss::PartialReduce all_ranks{
      [](void* ctx, double* buf, size_t count, hipStream_t st) -> int {
        return pbbss::comm_all_reduce_f64(static_cast<pbbss_handle_t>(ctx)->comm, buf, count, st);
      },
      h};
  const pbbss::PartialReduce* reduce = sharded ? &all_ranks : nullptr;
  // scalars per class of the spectral model's second parameter: concentration / variance (1),
  // per-dimension variances (E), covariance matrix (E * E)
  const size_t nscale = g_full ? (size_t)K * E * E : (g_diag ? (size_t)K * E : (size_t)K);
  if (o->covariance_norm < 0 || o->covariance_norm > 2) return PBBSS_ERR_INVALID_ARG;
  const bool has_gamma = gamma0 != nullptr;
  const bool has_model = in_eigvec && in_eigval && in_weight && in_mean && in_scale;
  if (has_gamma == has_model) return PBBSS_ERR_INVALID_ARG;
  if ((o->iterations == 0) != has_model) return PBBSS_ERR_INVALID_ARG;
  if (!out_eigvec || !out_eigval || !out_weight || !out_mean || !out_scale || !out_status)
    return PBBSS_ERR_INVALID_ARG;
  hipStream_t s = as_stream(stream);
  int64_t wb = 0, wk = 0, wt = 0;
  size_t wcount = 1;
  switch (o->weight_mode) {
    case PBBSS_JOINT_WEIGHT_FK: wb = K; wk = 1; wcount = (size_t)F * K; break;
    case PBBSS_JOINT_WEIGHT_K: wk = 1; wcount = K; break;
    case PBBSS_JOINT_WEIGHT_KT: wk = T; wt = 1; wcount = (size_t)K * T; break;
    default: break;
  }
  const size_t esz = o->embedding_is_f64 ? 8 : 4;
  // Rotated loop (round 4): ONE pass over the embedding per EM iteration -- the sweep kernel forms
  // the posteriors from the spatial quadratic forms Q and the spectral log-pdf of the SAME tile of
  // embedding rows it then accumulates the spectral M-step sums from, the spatial kernel runs
  // M-step, factorisation and the NEXT model's quadratic forms (embed.hip: joint_sweep_kernel,
  // cacgmm_em.hpp: run_joint_ms).  Served: vMF / spherical Gaussian, D <= 8, K <= 6, no inline
  // aligner, no fixed covariance; everything else keeps the three-kernel path below.
  // PBBSS_JOINT_ROTATED=0 switches it off (A/B runs, tests of the other path).
  static const bool rot_allowed = [] {
    const char* v = getenv("PBBSS_JOINT_ROTATED");
    return !(v && v[0] == '0');
  }();
  const bool rot = rot_allowed && !gen && !o->inline_pa && !(in_scale && gamma0) &&
                   o->iterations >= 2 &&
                   pbbss::joint_sweep_supported(o->kind, N, E, K, o->embedding_is_f64);
  const size_t np0 = wide ? pbbss::embed_wide_work_doubles(1, N, E, K)
                          : pbbss::embed_partial_doubles(1, N, E, K, nullptr);
  const size_t npj = rot ? pbbss::joint_sweep_partial_doubles(o->kind, N, E, K, o->embedding_is_f64) : 0;
  const size_t np = np0 > npj ? np0 : npj;
  const size_t nfkt = (size_t)F * K * T;
  const size_t nstate = (size_t)F * K * (D * D + 2);
  const size_t ngp = g_full ? pbbss::gauss_full_partial_doubles(1, N, E, K) : 0;
  const size_t nconst = g_diag ? pbbss::diag_consts_doubles(K, E) : 0;
  const size_t nmat = (size_t)F * K;
  const size_t ntmp = pbbss::joint_weight_tmp_doubles(o->weight_mode, F, K, T);
  const size_t ninv = gen ? pbbss::gen_state_doubles((int64_t)nmat, D) : 0;
  const size_t nyt = gen ? (size_t)F * T * D * (o->obs_is_c128 ? 16 : 8) : 0;
  char *yd, *g_yt;
  double *aff, *slp, *part, *offset, *prec, *tmp, *jstate, *wkn, *lpkn, *gpart, *mq, *dconst;
  double *lndet, *fin_tmp, *gshift, *g_mw, *g_cov, *g_inv, *g_logdet, *g_csum, *g_lp, *g_q;
  int32_t *gst, *g_zero;
  int rc = carve(h->work, [&](Carver& wc) {
    yd = wide ? nullptr : wc.take<char>((size_t)E * N * esz);  // (the class tiles read row-major)
    aff = wc.take<double>(nfkt);
    slp = wc.take<double>(nfkt);
    part = wc.take<double>(np);
    offset = wc.take<double>(K);
    prec = wc.take<double>(K);
    tmp = wc.take<double>(ntmp);
    jstate = wc.take<double>(nstate);
    wkn = g_full ? wc.take<double>(nfkt) : nullptr;   // (K, F*T) class weights
    lpkn = g_full ? wc.take<double>(nfkt) : nullptr;  // (K, F*T) log-pdf
    gpart = g_full ? wc.take<double>(ngp) : nullptr;
    mq = g_full ? wc.take<double>((size_t)K * E * E) : nullptr;
    dconst = g_diag ? wc.take<double>(nconst) : nullptr;
    gst = wc.take<int32_t>(16);                // status of the spectral half
    lndet = wc.take<double>((size_t)F * K);  // rotated loop: ln det B_fk of the current model
    fin_tmp = wc.take<double>((size_t)kJointFinHelpers * 2 * K * (E + 1));
    // sharded full covariance: the common shift of the first M-step
    gshift = wc.take<double>(pbbss::gauss_full_column_sums_doubles(E));
    // generic-size spatial half: M-step weights, covariances, inverse state, class sums,
    // zero-frame flags, frame-contiguous copy of the observation
    g_mw = gen ? wc.take<double>(nfkt) : nullptr;
    g_cov = gen ? wc.take<double>(nmat * D * D * 2) : nullptr;
    g_inv = gen ? wc.take<double>(ninv) : nullptr;
    g_logdet = gen ? wc.take<double>(nmat) : nullptr;
    g_csum = gen ? wc.take<double>(nmat) : nullptr;
    g_zero = gen ? wc.take<int32_t>((size_t)F) : nullptr;
    g_yt = gen ? wc.take<char>(nyt) : nullptr;
    g_lp = (gen && o->inline_pa) ? wc.take<double>(nfkt) : nullptr;  // spatial log-pdf
    g_q = (gen && o->inline_pa) ? wc.take<double>(nfkt) : nullptr;   // quadratic forms
  });
  if (rc != PBBSS_OK) return rc;
  if (hipMemsetAsync(gst, 0, 64, as_stream(stream)) != hipSuccess) return PBBSS_ERR_HIP;
  TimedRegion tr(h, s);
  if (wide && !g_full) {  // the Gaussians' common shift, once per fit
    rc = pbbss::embed_wide_shift(o->kind, embedding, o->embedding_is_f64, 1, N, E, K, part, s);
    if (rc != PBBSS_OK) return rc;
  }
  if (!wide) {
    rc = pbbss::launch_embed_prepare(embedding, o->embedding_is_f64, 1, N, E, 0, yd, nullptr, s);
    if (rc != PBBSS_OK) return rc;
  }
  if (sharded && g_full) {
    // the first M-step has no previous means to centre on, and every rank must subtract the same
    // point: the column mean of ALL ranks' embedding rows (column sums and row counts all-reduced)
    rc = pbbss::launch_gauss_full_column_sums(embedding, o->embedding_is_f64, N, E, gshift, s);
    if (rc != PBBSS_OK) return rc;
    if ((rc = all_ranks.fn(all_ranks.ctx, gshift, (size_t)E + 1, s)) != PBBSS_OK) return rc;
    if ((rc = pbbss::launch_gauss_full_column_mean(gshift, E, s)) != PBBSS_OK) return rc;
  }
  if (has_model) {
    if ((rc = copy_d2d(out_eigvec, in_eigvec, (size_t)F * K * D * D * 16, s)) != PBBSS_OK) return rc;
    if ((rc = copy_d2d(out_eigval, in_eigval, (size_t)F * K * D * 8, s)) != PBBSS_OK) return rc;
    if ((rc = copy_d2d(out_weight, in_weight, wcount * 8, s)) != PBBSS_OK) return rc;
    if ((rc = copy_d2d(out_mean, in_mean, (size_t)K * E * 8, s)) != PBBSS_OK) return rc;
    if ((rc = copy_d2d(out_scale, in_scale, nscale * 8, s)) != PBBSS_OK) return rc;
  }
  // spectral log-pdf (times spectral_weight) of every point, laid out (F,K,T)
  const bool fixed_scale = in_scale && has_gamma;
  bool mq_fresh = false;  // the full-covariance M-step also leaves the factorisation behind
  auto spectral = [&]() -> int {
    if (wide && !g_full)
      return pbbss::embed_wide_log_pdf(o->kind, embedding, o->embedding_is_f64, 1, N, E, K, out_mean,
                                       out_scale, o->spectral_weight, T, part, slp,
                                       h->cfg.lds_limit, s, /*have_shift=*/true);
    if (g_diag)
      return pbbss::launch_diag_estep(yd, o->embedding_is_f64, N, E, K, out_mean, out_scale,
                                      o->spectral_weight, T, dconst, slp, s);
    if (g_full) {
      int r = PBBSS_OK;
      if (!mq_fresh || fixed_scale)
        r = pbbss::launch_gauss_full_factor(out_scale, K, E, mq, offset, gst, s);
      if (r != PBBSS_OK) return r;
      r = pbbss::launch_gauss_full_logpdf(embedding, o->embedding_is_f64, 1, N, E, K, out_mean, mq,
                                          offset, nullptr, lpkn, nullptr, s);
      if (r != PBBSS_OK) return r;
      return pbbss::launch_kn_to_fkt(lpkn, o->spectral_weight, F, K, T, slp, s);
    }
    if (fixed_scale || o->iterations == 0) {  // otherwise the M-step finalize wrote them
      int r = pbbss::launch_embed_offsets(o->kind, K, E, out_scale, offset, prec, s);
      if (r != PBBSS_OK) return r;
    }
    return pbbss::launch_embed_estep(o->kind, yd, o->embedding_is_f64, 1, N, E, K, out_mean, prec,
                                     offset, nullptr, o->spectral_weight, T, slp, nullptr, s);
  };
  // generic-size spatial half: the posteriors of the current model (E-step of gcacgmm.py:66-117
  // with the spectral log-pdf as the extra exponent), then the cACG M-step from them
  auto class_weights = [&](const double* a) -> int {
    if (wide)
      return pbbss::embed_wide_joint_weight(o->weight_mode, a, saliency, F, K, T, tmp, out_weight, s);
    return pbbss::launch_joint_weight(o->weight_mode, a, saliency, F, K, T, tmp, out_weight, s,
                                      reduce);
  };
  const pbbss::GenInverseState g_state{g_inv, g_logdet, nullptr};
  auto gen_m_step = [&](const double* gam, bool fk_weights) -> int {
    int r = pbbss::launch_gen_mstep_cov(observation, o->obs_is_c128, F, T, D, K, g_mw, gam, saliency,
                                        PBBSS_WEIGHT_PER_CLASS_MEAN, g_csum, g_cov,
                                        fk_weights ? out_weight : tmp, s);
    if (r != PBBSS_OK) return r;
    return pbbss::launch_gen_heev(g_cov, (int64_t)nmat, D, o->covariance_norm, o->eigenvalue_floor,
                                  out_eigval, static_cast<double*>(out_eigvec), out_status,
                                  h->cfg.lds_limit, s);
  };
  auto gen_e_step = [&](double* aff_out, double eps, bool for_m_step, int inline_pa) -> int {
    pbbss::GenEstepArgs e{g_yt, o->obs_is_c128, PBBSS_LAYOUT_DT, F, T, D, K,
                          static_cast<const double*>(out_eigvec), out_eigval, out_weight, wb, wk,
                          wt};
    e.raw_dt = 1;
    if (inline_pa) {
      // spatial log-pdf and quadratic forms first, then the per-bin permutation search
      e.out_q = g_q;
      e.out_logpdf = g_lp;
      int r = pbbss::launch_gen_estep(e, g_state, s);
      if (r != PBBSS_OK) return r;
      return pbbss::launch_gen_joint_pa(g_yt, o->obs_is_c128, F, T, D, K, g_lp, g_q, slp,
                                        o->spatial_weight, out_weight, wb, wk, wt, saliency, eps,
                                        aff_out, for_m_step ? g_mw : nullptr,
                                        for_m_step ? g_zero : nullptr, s);
    }
    e.eps = eps;
    e.out_aff = aff_out;
    e.saliency = saliency;
    e.out_mweight = for_m_step ? g_mw : nullptr;
    e.out_zero = for_m_step ? g_zero : nullptr;
    e.extra = slp;
    e.spatial_scale = o->spatial_weight;
    return pbbss::launch_gen_estep(e, g_state, s);
  };
  if (gen) {
    if ((rc = pbbss::launch_gen_transpose(observation, o->obs_is_c128, F, T, D, g_yt, s)) != PBBSS_OK)
      return rc;
    if (hipMemsetAsync(out_status, 0, nmat * sizeof(int32_t), s) != hipSuccess) return PBBSS_ERR_HIP;
    if (hipMemsetAsync(g_zero, 0, (size_t)F * sizeof(int32_t), s) != hipSuccess) return PBBSS_ERR_HIP;
  }
  // what every fused spatial launch of this fit has in common: one M-step over the bins of the
  // observation, the model in the caller's output arrays
  auto spatial_args = [&]() {
    pbbss::EmArgs a{};
    a.y = observation;
    a.B = F;
    a.T = T;
    a.saliency = saliency;
    a.out_eigvec = static_cast<double*>(out_eigvec);
    a.out_eigval = out_eigval;
    a.out_status = out_status;
    a.iterations = 1;
    a.covariance_norm = o->covariance_norm;
    a.weight_mode = PBBSS_WEIGHT_PER_CLASS_MEAN;
    a.layout = PBBSS_LAYOUT_TD;
    a.eig_floor = o->eigenvalue_floor;
    return a;
  };
  auto joint = [&](int iterations, double* aff_out, int inline_pa, const double* state_in,
                   double* state_out, int emit_model) -> int {
    if (gen) {
      int r = gen_e_step(aff_out, iterations > 0 ? o->affiliation_eps : 0.0, iterations > 0,
                         inline_pa);
      if (r != PBBSS_OK || iterations == 0) return r;
      return gen_m_step(aff_out, o->weight_mode == PBBSS_JOINT_WEIGHT_FK);
    }
    pbbss::EmArgs a = spatial_args();
    a.in_eigvec = static_cast<const double*>(out_eigvec);  // in place: one workgroup per bin
    a.in_eigval = out_eigval;
    a.in_weight = out_weight;
    a.wb = wb;
    a.wk = wk;
    a.wt = wt;
    a.out_aff = aff_out;
    a.iterations = iterations;
    a.aff_eps = o->affiliation_eps;
    pbbss::JointExtras jx{slp, o->spatial_weight, nullptr, state_in, state_out, emit_model,
                          (iterations > 0 && o->weight_mode == PBBSS_JOINT_WEIGHT_FK) ? out_weight
                                                                                     : nullptr};
    return pbbss::joint_launch(D, K, o->obs_is_c128, a, jx, inline_pa, h->cfg, s);
  };
  // spatial half of the rotated loop: mode 0 = quadratic forms of the eigen model in the output
  // arrays, 1 = M-step from (G = aff, Q = slp) + factorisation + quadratic forms of the new
  // model (Q in place), 2 = M-step + exact eigen path, (V, lambda) emitted (last iteration)
  // in-launch finalize: not for sharded fits (the all-reduce of the partials has to sit between
  // the sweep and the finalize, in stream order); PBBSS_JOINT_INLAUNCH_FINALIZE=0 for A/B runs
  static const bool fin_allowed = [] {
    const char* v = getenv("PBBSS_JOINT_INLAUNCH_FINALIZE");
    return !(v && v[0] == '0');
  }();
  const bool fin_in_launch = rot && fin_allowed && !reduce && h->cfg.xbuf &&
                             2 * K * (E + 1) <= pbbss::kSpectralFinMaxW2;
  auto spatial_ms = [&](int mode) -> int {
    pbbss::EmArgs a = spatial_args();
    a.gamma0 = mode == 0 ? nullptr : aff;
    a.q0 = mode == 0 ? nullptr : slp;
    a.in_eigvec = static_cast<const double*>(out_eigvec);
    a.in_eigval = out_eigval;
    pbbss::JointMs jm{};
    jm.mode = mode;
    jm.q_out = slp;
    jm.lndet_out = lndet;
    jm.weight_fk_out = (mode != 0 && o->weight_mode == PBBSS_JOINT_WEIGHT_FK) ? out_weight : nullptr;
    jm.fin.kind = -1;
    if (mode != 0 && fin_in_launch) {
      int C = 0;
      pbbss::joint_sweep_chunks(o->kind, N, E, K, o->embedding_is_f64, &C);
      jm.fin = pbbss::SpectralFin{o->kind == PBBSS_EMBED_VMF ? 0 : 1, joint_fin_helpers(), C, E, K,
                                  part, fin_tmp,
                                  reinterpret_cast<unsigned*>(h->cfg.xbuf + 224),  // free word
                                  o->min_concentration, o->max_concentration, out_mean, out_scale,
                                  offset, prec};
      if (jm.fin.helpers > C) jm.fin.helpers = C;
    }
    return pbbss::joint_ms_launch(D, K, o->obs_is_c128, a, jm, h->cfg, s);
  };
  for (int it = 0; it < o->iterations; ++it) {
    const double* src = gamma0;
    if (it == 0 && gen) {
      rc = pbbss::launch_gen_init_weights(g_yt, o->obs_is_c128, PBBSS_LAYOUT_DT, F, T, D, K, gamma0,
                                          saliency, g_mw, g_zero, s);
      if (rc != PBBSS_OK) return rc;
      if ((rc = gen_m_step(gamma0, false)) != PBBSS_OK) return rc;
    } else if (it == 0) {
      // first M-step from the initial affiliations, quadratic form = 1 (gcacgmm.py:194-196)
      pbbss::EmArgs a = spatial_args();
      a.gamma0 = gamma0;
      rc = pbbss::em_launch(D, K, o->obs_is_c128, a, h->cfg, s);
      if (rc != PBBSS_OK) return rc;
    } else if (rot) {
      // sweep: posteriors of the current model -> aff, spectral sums -> part; then the spectral
      // finalize and the spatial M-step / factorisation / next quadratic forms
      rc = pbbss::launch_joint_sweep(o->kind, embedding, o->embedding_is_f64, F, T, E, K, D, slp,
                                     lndet, out_weight, wb, wk, wt, out_mean, prec, offset, o->spatial_weight,
                                     o->spectral_weight, saliency, o->affiliation_eps, aff, part, s);
      if (rc != PBBSS_OK) return rc;
      // The spectral finalize (ONE workgroup walking the chunk partials: 14-18 us) and the spatial
      // kernel are independent -- both only feed the NEXT sweep -- so the finalize runs beside
      // the spatial kernel on the handle's side stream (fork after the sweep, join before the
      // next sweep).  Sharded fits keep it in stream order (the all-reduce of the partials is
      // enqueued on the caller's stream).  PBBSS_JOINT_SIDE_FINALIZE=0: in stream order (A/B).
      static const bool side_allowed = [] {
        const char* v = getenv("PBBSS_JOINT_SIDE_FINALIZE");
        return !(v && v[0] == '0');
      }();
      const bool side = side_allowed && !reduce && h->cfg.side_stream && !fin_in_launch;
      hipStream_t fs = s;
      if (side) {
        if ((rc = pbbss::side_fork(h->cfg, s)) != PBBSS_OK) return rc;
        fs = h->cfg.side_stream;
      }
      // The finalize goes onto the side stream BEFORE the spatial kernel is enqueued and the
      // caller's stream waits for it only after the class weights, so with_side_stream's order
      // does not fit: the two halves of the join, under its error policy -- once forked, the
      // join is issued whatever fails in between, and the first error is returned.
      if (!fin_in_launch) {
        rc = pbbss::launch_joint_sweep_finalize(o->kind, embedding, o->embedding_is_f64, N, E, K,
                                                o->min_concentration, o->max_concentration, part,
                                                out_mean, out_scale, offset, prec, fs, reduce);
      }
      int rc_join = side ? pbbss::side_join_record(h->cfg) : PBBSS_OK;
      if (rc == PBBSS_OK) rc = spatial_ms(it == o->iterations - 1 ? 2 : 1);
      if (rc == PBBSS_OK && o->weight_mode != PBBSS_JOINT_WEIGHT_FK) {
        rc = pbbss::launch_joint_weight(o->weight_mode, aff, saliency, F, K, T, tmp, out_weight, s,
                                        reduce);
      }
      if (side && rc_join == PBBSS_OK) rc_join = pbbss::side_join_wait(h->cfg, s);
      if (rc != PBBSS_OK || rc_join != PBBSS_OK) return rc != PBBSS_OK ? rc : rc_join;
      continue;
    } else {
      if ((rc = spectral()) != PBBSS_OK) return rc;
      // the model travels as packed inverse covariances between iterations; the first joint
      // step reads the eigen model of the initial M-step, the last one emits (V, lambda)
      const bool last = (it == o->iterations - 1);
      rc = joint(1, aff, o->inline_pa, it == 1 ? nullptr : jstate, last ? nullptr : jstate,
                 last ? 1 : 0);
      if (rc != PBBSS_OK) return rc;
      src = aff;
    }
    if (it == 0 || o->weight_mode != PBBSS_JOINT_WEIGHT_FK) {  // 'fk' weights: joint kernel
      if ((rc = class_weights(src)) != PBBSS_OK) return rc;
    }
    if (g_full) {
      // GaussianTrainer._fit(covariance_type='full') on the (1, F*T, E) embedding with the masked
      // affiliations as (K, F*T) class weights (gcacgmm.py:297-307); the kernel leaves mean,
      // covariance and the factorisation the next E-step needs
      if ((rc = pbbss::launch_fkt_to_kn(src, saliency, F, K, T, wkn, s)) != PBBSS_OK) return rc;
      rc = pbbss::launch_gauss_full_fit(embedding, o->embedding_is_f64, 1, N, E, K, wkn, nullptr,
                                        gpart, out_mean, out_scale, mq, offset, nullptr, gst, s,
                                        it > 0 ? out_mean : nullptr,  // about the previous means
                                        (sharded && it == 0) ? gshift : nullptr, reduce);
      mq_fresh = true;
    } else if (wide) {
      rc = pbbss::embed_wide_fit(o->kind, embedding, o->embedding_is_f64, 1, N, E, K, src, 0,
                                 o->min_concentration, o->max_concentration, part, out_mean,
                                 out_scale, h->cfg.lds_limit, s, T, saliency, /*have_shift=*/true);
    } else {
      rc = pbbss::launch_embed_fit(o->kind, embedding, o->embedding_is_f64, 1, N, E, K, src, T,
                                   saliency, o->min_concentration, o->max_concentration, -1, part,
                                   out_mean, out_scale, nullptr, g_diag ? nullptr : offset,
                                   g_diag ? nullptr : prec, it == 0 ? 0 : 1, s, nullptr, reduce);
    }
    if (rc != PBBSS_OK) return rc;
    if (fixed_scale) {  // fixed_covariance (gcacgmm.py:305-312)
      if ((rc = copy_d2d(out_scale, in_scale, nscale * 8, s)) != PBBSS_OK) return rc;
    }
    if (rot && it == 0) {  // quadratic forms of the first model for the first sweep
      if ((rc = spatial_ms(0)) != PBBSS_OK) return rc;
    }
  }
  if (o->final_predict && out_affiliation) {
    if ((rc = spectral()) != PBBSS_OK) return rc;
    if ((rc = joint(0, out_affiliation, 0, nullptr, nullptr, 0)) != PBBSS_OK) return rc;
  }
  // a spectral covariance that stopped being positive definite (the reference raises from
  // sklearn's precision Cholesky, gaussian.py:26): PBBSS_ST_NOT_POSDEF in status word 0
  if (g_full) return pbbss::launch_or_status(gst, out_status, s);
  return PBBSS_OK;
}
