// extern "C" boundary of libpbbss_hip.so (see include/pbbss.h): argument validation, handle
// state (handle.hip), kernel dispatch, and the stream-ordered launch sequences of the multi-kernel
// fits (the joint models: capi_joint.hip).  No device code lives in this layer.
#include "handle.hpp"
#include "beamform.hpp"
#include "dhtv.hpp"
#include "gauss_full.hpp"
#include "generic.hpp"
#include "generic_bf.hpp"
#include "stft.hpp"
#include "cbmm_launch.hpp"
#include "initializer.hpp"
#include "comm.hpp"

using pbbss::as_stream, pbbss::copy_d2d, pbbss::embed_shape_ok, pbbss::Carver, pbbss::carve,
    pbbss::DeviceGuard, pbbss::TimedRegion, pbbss::ResidencyGate;

// ---------------------------------------------------------------------------
// Multi-GPU: RCCL communicator in the handle + the mask all-gather (comm.hip)
// ---------------------------------------------------------------------------
PBBSS_API int pbbss_comm_unique_id(void* out_id) {
  if (!out_id) return PBBSS_ERR_INVALID_ARG;
  return pbbss::comm_unique_id(out_id);
}

PBBSS_API int pbbss_comm_create(pbbss_handle_t h, const void* unique_id, int world_size, int rank) {
  DeviceGuard device_guard(h);
  if (!h || !unique_id || world_size < 1 || rank < 0 || rank >= world_size)
    return PBBSS_ERR_INVALID_ARG;
  if (h->comm) return PBBSS_ERR_INVALID_ARG;  // one communicator per handle
  void* c = nullptr;
  const int rc = pbbss::comm_create(unique_id, world_size, rank, &c);
  if (rc != PBBSS_OK) return rc;
  h->comm = c;
  h->comm_world = world_size;
  h->comm_rank = rank;
  return PBBSS_OK;
}

PBBSS_API int pbbss_comm_destroy(pbbss_handle_t h) {
  DeviceGuard device_guard(h);
  if (!h) return PBBSS_ERR_INVALID_ARG;
  // collectives enqueued on any stream of this device finish before their buffers go away
  if (h->comm) (void)hipDeviceSynchronize();
  const int rc = pbbss::comm_destroy(h->comm);
  h->comm = nullptr;
  h->comm_world = 1;
  h->comm_rank = 0;
  h->comm_buf.release();
  return rc;
}

PBBSS_API int pbbss_comm_info(pbbss_handle_t h, int* out_world_size, int* out_rank) {
  if (!h || !out_world_size || !out_rank) return PBBSS_ERR_INVALID_ARG;
  if (!h->comm) return PBBSS_ERR_INVALID_ARG;  // pbbss_comm_create first
  return pbbss::comm_query(h->comm, out_world_size, out_rank);
}

PBBSS_API int pbbss_shard_bounds(int64_t total_bins, int world_size, int rank, int64_t* out_start,
                                 int64_t* out_stop) {
  if (total_bins < 0 || world_size < 1 || rank < 0 || rank >= world_size || !out_start || !out_stop)
    return PBBSS_ERR_INVALID_ARG;
  const int64_t base = total_bins / world_size, extra = total_bins % world_size;
  *out_start = rank * base + (rank < extra ? rank : extra);
  *out_stop = *out_start + base + (rank < extra ? 1 : 0);
  return PBBSS_OK;
}

PBBSS_API int pbbss_allgather_unpack(pbbss_handle_t h, const void* gathered, int elem_bytes,
                                     int world_size, int64_t outer, int64_t total_bins,
                                     int64_t inner, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !gathered || !out || world_size < 1 || outer < 0 || total_bins < 0 || inner < 0)
    return PBBSS_ERR_INVALID_ARG;
  if (elem_bytes != 4 && elem_bytes != 8) return PBBSS_ERR_UNSUPPORTED;
  return pbbss::launch_allgather_unpack(gathered, elem_bytes, world_size, outer, total_bins, inner,
                                        out, as_stream(stream));
}

PBBSS_API int pbbss_allgather_masks(pbbss_handle_t h, const void* local, int elem_bytes,
                                    int64_t outer, int64_t total_bins, int64_t inner, void* out,
                                    void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !out || outer < 0 || total_bins < 0 || inner < 0) return PBBSS_ERR_INVALID_ARG;
  if (elem_bytes != 4 && elem_bytes != 8) return PBBSS_ERR_UNSUPPORTED;
  if (!h->comm) return PBBSS_ERR_INVALID_ARG;  // pbbss_comm_create first
  const int world = h->comm_world;
  int64_t lo = 0, hi = 0;
  (void)pbbss_shard_bounds(total_bins, world, h->comm_rank, &lo, &hi);
  const int64_t nloc = hi - lo, pad = (total_bins + world - 1) / world;
  if (nloc > 0 && !local) return PBBSS_ERR_INVALID_ARG;
  const size_t block = (size_t)outer * pad * inner * elem_bytes;
  if (block == 0) return PBBSS_OK;
  // The pack / gather buffers belong to the communicator (grow-only, released by
  // pbbss_comm_destroy / pbbss_destroy): the work slab may be re-carved or reallocated by the next
  // library call on another stream while this collective is still in flight.
  char *packed, *gathered;
  int rc = carve(h->comm_buf, [&](Carver& wc) {
    packed = wc.take<char>(block);
    gathered = wc.take<char>(block * world);
  });
  if (rc != PBBSS_OK) return rc;
  hipStream_t s = as_stream(stream);
  rc = pbbss::launch_allgather_pack(local, elem_bytes, outer, nloc, pad, inner, packed, s);
  if (rc != PBBSS_OK) return rc;
  rc = pbbss::comm_all_gather_bytes(h->comm, packed, gathered, block, s);
  if (rc != PBBSS_OK) return rc;
  return pbbss::launch_allgather_unpack(gathered, elem_bytes, world, outer, total_bins, inner, out,
                                        s);
}

PBBSS_API int pbbss_normalize_observation(pbbss_handle_t h, const void* y, int is_c128,
                                          int64_t B, int T, int D, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !out || B <= 0 || T <= 0 || D <= 0) return PBBSS_ERR_INVALID_ARG;
  for (int64_t b0 = 0; b0 < B; b0 += 65535) {  // grid.y limit: split the batch
    int64_t nb = (B - b0 < 65535) ? (B - b0) : 65535;
    size_t esz = is_c128 ? 16 : 8;
    int rc = pbbss::launch_normalize((const char*)y + (size_t)b0 * T * D * esz, is_c128, nb, T, D,
                                     (char*)out + (size_t)b0 * T * D * esz, as_stream(stream));
    if (rc != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}

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
    // generic-size path (generic.hip; also more than 6 classes at any D): E-step, covariance + weights, eigendecomposition per
    // iteration, enqueued back to back; the model lives in the caller's output buffers
    if (!pbbss::gen_em_supported(D, K)) return PBBSS_ERR_UNSUPPORTED;
    if (o->layout != PBBSS_LAYOUT_TD) return PBBSS_ERR_UNSUPPORTED;
    hipStream_t s = as_stream(stream);
    const size_t nkt = (size_t)B * K * T;
    const size_t nmat = (size_t)B * K;
    const size_t ninv = pbbss::gen_state_doubles((int64_t)nmat, D);
    const size_t ny = (size_t)B * T * D * (o->y_is_c128 ? 16 : 8);
    const bool transpose = B <= 65535;  // frame-contiguous copy for the E-steps of the loop
    double *aff, *mw, *cov, *inv, *inv_logdet, *csum;
    int32_t *inv_ok, *zero_bin;
    char* yt;
    const int rc_work = carve(h->work, [&](Carver& wc) {
      aff = wc.take<double>(nkt);
      mw = wc.take<double>(nkt);  // M-step weights gamma sal / q / |y|^2 of every frame
      cov = wc.take<double>(nmat * D * D * 2);
      inv = wc.take<double>(ninv);
      inv_logdet = wc.take<double>(nmat);
      inv_ok = wc.take<int32_t>(nmat);
      zero_bin = wc.take<int32_t>((size_t)B);
      csum = wc.take<double>(nmat);
      yt = transpose ? wc.take<char>(ny) : nullptr;
    });
    if (rc_work != PBBSS_OK) return rc_work;
    TimedRegion tr(h, s);
    const size_t ysz = o->y_is_c128 ? 16 : 8;
    const size_t ld2 = pbbss::gen_state_doubles(1, D);
    // One chain of launches for the bins [b0, b0 + nb): every array is sliced along the bins
    // (nothing couples them under the per-bin weight modes of this entry point).
    auto chain = [&](int64_t b0, int64_t nb, hipStream_t st) -> int {
      const size_t m0 = (size_t)b0 * K, nm = (size_t)nb * K;
      const char* y_c = static_cast<const char*>(y) + (size_t)b0 * T * D * ysz;
      const double* gamma0_c = gamma0 ? gamma0 + m0 * T : nullptr;
      const double* sal_c = saliency ? saliency + (size_t)b0 * T : nullptr;
      const uint8_t* act_c = activity ? activity + m0 * T : nullptr;
      double* evec_c = static_cast<double*>(out_eigvec) + m0 * D * D * 2;
      double* eval_c = out_eigval + m0 * D;
      double* w_c = out_weight + m0;
      int32_t* st_c = out_status + m0;
      double* aff_c = aff + m0 * T;
      double* mw_c = mw + m0 * T;
      double* cov_c = cov + m0 * D * D * 2;
      double* csum_c = csum + m0;
      int32_t* zero_c = zero_bin + b0;
      int32_t* ok_c = inv_ok + m0;
      const pbbss::GenInverseState state{inv + m0 * ld2, inv_logdet + m0, ok_c};
      const pbbss::GenInverseState state_from_eig{inv + m0 * ld2, inv_logdet + m0, nullptr};
      int rc;
      if (has_model) {
        if ((rc = copy_d2d(evec_c, static_cast<const double*>(in_eigvec) + m0 * D * D * 2,
                           nm * D * D * 16, st)) != PBBSS_OK) return rc;
        if ((rc = copy_d2d(eval_c, in_eigval + m0 * D, nm * D * 8, st)) != PBBSS_OK) return rc;
        if ((rc = copy_d2d(w_c, in_weight + m0, nm * 8, st)) != PBBSS_OK) return rc;
      }
      if (hipMemsetAsync(st_c, 0, nm * sizeof(int32_t), st) != hipSuccess) return PBBSS_ERR_HIP;
      // bins with an all-zero frame (flagged by the E-step / the initial weights) never take
      // the inverse fast path
      if (hipMemsetAsync(zero_c, 0, (size_t)nb * sizeof(int32_t), st) != hipSuccess) return PBBSS_ERR_HIP;
      // E-steps read a (B, D, T) copy of the raw observation (lane = frame is then the contiguous
      // axis); the covariance kernel keeps the caller's (B, T, D) array (its lanes span the channels)
      const void* y_e = y_c;
      int layout_e = PBBSS_LAYOUT_TD;
      if (transpose) {
        char* yt_c = yt + (size_t)b0 * T * D * ysz;
        if ((rc = pbbss::launch_gen_transpose(y_c, o->y_is_c128, nb, T, D, yt_c, st)) != PBBSS_OK) return rc;
        y_e = yt_c;
        layout_e = PBBSS_LAYOUT_DT;
      }
      for (int it = 0; it < o->iterations; ++it) {
        const double* g_src = gamma0_c;
        if (it > 0 || has_model) {
          // from the second iteration on, classes whose inverse was accepted skip (V, lambda)
          rc = pbbss::launch_gen_estep(y_e, o->y_is_c128, layout_e, nb, T, D, K, evec_c, eval_c, w_c,
                                       K, 1, 0, act_c, o->affiliation_eps, aff_c, nullptr, nullptr,
                                       st, it > 0 ? state : state_from_eig, sal_c, mw_c, zero_c,
                                       /*raw_dt=*/1);
          if (rc != PBBSS_OK) return rc;
          g_src = aff_c;
        } else {
          rc = pbbss::launch_gen_init_weights(y_e, o->y_is_c128, layout_e, nb, T, D, K, gamma0_c,
                                              sal_c, mw_c, zero_c, st);
          if (rc != PBBSS_OK) return rc;
        }
        rc = pbbss::launch_gen_mstep_cov(y_c, o->y_is_c128, nb, T, D, K, mw_c, g_src, sal_c,
                                         o->weight_mode, csum_c, cov_c, w_c, st);
        if (rc != PBBSS_OK) return rc;
        const bool last = it + 1 == o->iterations;
        if (!last && !o->force_eig) {
          rc = pbbss::launch_gen_inverse(cov_c, (int64_t)nm, D, o->eigenvalue_floor, state.inv,
                                         state.logdet, ok_c, st, zero_c, K);
          if (rc != PBBSS_OK) return rc;
        } else if (!last) {
          if (hipMemsetAsync(ok_c, 0, nm * sizeof(int32_t), st) != hipSuccess) return PBBSS_ERR_HIP;
        }
        // the eigendecomposition the caller sees comes from the last iteration; before that it
        // only runs for the matrices the inverse test rejected.  Status words are those of the
        // last iteration (earlier ones are overwritten).
        rc = pbbss::launch_gen_heev(cov_c, (int64_t)nm, D, o->covariance_norm, o->eigenvalue_floor,
                                    eval_c, evec_c, st_c, h->cfg.lds_limit, st, last ? nullptr : ok_c);
        if (rc != PBBSS_OK) return rc;
      }
      if (o->final_predict && (out_affiliation || out_quadratic_form)) {
        rc = pbbss::launch_gen_estep(y_e, o->y_is_c128, layout_e, nb, T, D, K, evec_c, eval_c, w_c, K,
                                     1, 0, nullptr, 0.0,
                                     out_affiliation ? out_affiliation + m0 * T : nullptr,
                                     out_quadratic_form ? out_quadratic_form + m0 * T : nullptr,
                                     nullptr, st, state_from_eig, nullptr, nullptr, nullptr,
                                     /*raw_dt=*/1);
        if (rc != PBBSS_OK) return rc;
      }
      return PBBSS_OK;
    };
    // 2^n + 1 bins (every standard STFT size): the last bin turns a whole number of residency
    // rounds into that number plus one straggler in EVERY kernel of the loop (513 bins x 8
    // E-step wavefronts = 4104 on 4096 slots; 513 x 6 covariance workgroups on 768 slots).  A few
    // remainder bins therefore run as their own chain on the side stream, concurrently with the
    // main chain -- forked once, joined once: the bins do not interact inside the loop.
    const int64_t per_round = h->cfg.num_cu > 0 ? h->cfg.num_cu : 256;
    const int64_t rem = B % per_round;
    const bool peel = h->cfg.side_stream && h->cfg.allow_split && B > per_round && rem > 0 &&
                      rem * 16 <= per_round;
    if (!peel) return chain(0, B, s);
    if (hipEventRecord(h->cfg.ev_fork, s) != hipSuccess) return PBBSS_ERR_HIP;
    if (hipStreamWaitEvent(h->cfg.side_stream, h->cfg.ev_fork, 0) != hipSuccess) return PBBSS_ERR_HIP;
    int rc = chain(0, B - rem, s);
    const int rc2 = chain(B - rem, rem, h->cfg.side_stream);
    // join even after an error on one side: the caller's stream must cover everything enqueued
    if (hipEventRecord(h->cfg.ev_join, h->cfg.side_stream) != hipSuccess) return PBBSS_ERR_HIP;
    if (hipStreamWaitEvent(s, h->cfg.ev_join, 0) != hipSuccess) return PBBSS_ERR_HIP;
    return rc != PBBSS_OK ? rc : rc2;
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
    return pbbss::launch_gen_estep(y, y_is_c128, layout, B, T, D, K,
                                   static_cast<const double*>(eigvec), eigval, weight, wb, wk, wt,
                                   activity, affiliation_eps, out_affiliation, out_quadratic_form,
                                   out_log_pdf, as_stream(stream),
                                   pbbss::GenInverseState{inv, inv_logdet, nullptr});
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
    // generic-size path (generic_watson.hip): per iteration class log-pdfs -> softmax with the
    // weights -> masked covariance of the unit-norm frames + weights -> eigh -> principal pair,
    // concentration, ln c; enqueued back to back, the model lives in the work area
    if (!pbbss::gen_supported(D, K) || B > 65535) return PBBSS_ERR_UNSUPPORTED;
    hipStream_t s = as_stream(stream);
    const size_t nkt = (size_t)B * K * T, nmat = (size_t)B * K;
    double *aff, *lp, *cov, *evec, *eval, *mode_w, *conc_w, *weight_w, *lognorm;
    int32_t* status_w;
    int rc = carve(h->work, [&](Carver& wc) {
      aff = wc.take<double>(nkt);
      lp = wc.take<double>(nkt);
      cov = wc.take<double>(nmat * D * D * 2);
      evec = wc.take<double>(nmat * D * D * 2);
      eval = wc.take<double>(nmat * D);
      mode_w = wc.take<double>(nmat * D * 2);
      conc_w = wc.take<double>(nmat);
      weight_w = wc.take<double>(nmat);
      lognorm = wc.take<double>(nmat);
      status_w = wc.take<int32_t>(nmat);
    });
    if (rc != PBBSS_OK) return rc;
    double* mode = out_mode ? static_cast<double*>(out_mode) : mode_w;
    double* conc = out_concentration ? out_concentration : conc_w;
    double* weight = out_weight ? out_weight : weight_w;
    int32_t* status = out_status ? out_status : status_w;
    const pbbss::GenWatsonSpline sp{spline_t, spline_c, o->n_coef, o->ev_min, o->ev_max,
                                    o->max_concentration};
    TimedRegion tr(h, s);
    if (hipMemsetAsync(status, 0, nmat * sizeof(int32_t), s) != hipSuccess) return PBBSS_ERR_HIP;
    if (has_model) {
      if ((rc = copy_d2d(mode, in_mode, nmat * D * 16, s)) != PBBSS_OK) return rc;
      if ((rc = copy_d2d(conc, in_concentration, nmat * 8, s)) != PBBSS_OK) return rc;
      if ((rc = copy_d2d(weight, in_weight, nmat * 8, s)) != PBBSS_OK) return rc;
      if ((rc = pbbss::launch_gen_watson_lognorm(conc, (int64_t)nmat, D, lognorm, s)) != PBBSS_OK)
        return rc;
    }
    auto e_step = [&](double* out_lp, double* out_aff) {
      int r = pbbss::launch_gen_watson_logpdf(y, o->y_is_c128, B, T, D, K, mode, conc, lognorm,
                                              out_lp, s);
      if (r != PBBSS_OK || !out_aff) return r;
      return pbbss::launch_log_pdf_to_affiliation(out_lp, B, K, T, weight, K, 1, 0, nullptr, 0.0,
                                                  out_aff, s);
    };
    for (int it = 0; it < o->iterations; ++it) {
      const double* g_src = gamma0;
      if (it > 0 || has_model) {
        if ((rc = e_step(lp, aff)) != PBBSS_OK) return rc;
        g_src = aff;
      }
      rc = pbbss::launch_gen_cov(y, o->y_is_c128, PBBSS_LAYOUT_TD, B, T, D, K, g_src,
                                 (int64_t)K * T, nullptr, saliency, /*mode=*/3, o->weight_mode, cov,
                                 weight, nullptr, h->cfg.lds_limit, s);
      if (rc != PBBSS_OK) return rc;
      rc = pbbss::launch_gen_heev(cov, (int64_t)nmat, D, -1, 0.0, eval, evec, status,
                                  h->cfg.lds_limit, s);
      if (rc != PBBSS_OK) return rc;
      rc = pbbss::launch_gen_watson_finish(eval, evec, (int64_t)nmat, D, sp, mode, conc, lognorm, s);
      if (rc != PBBSS_OK) return rc;
    }
    if (o->final_predict && (out_affiliation || out_log_pdf))
      return e_step(out_log_pdf ? out_log_pdf : lp, out_affiliation);
    return PBBSS_OK;
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

// ---------------------------------------------------------------------------
// N2: real-embedding mixtures (the joint spatial+spectral models: capi_joint.hip).
// These are multi-kernel loops enqueued asynchronously on `stream` (no host sync).
// ---------------------------------------------------------------------------
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
  hipStream_t s = as_stream(stream);
  const size_t np = pbbss::gauss_full_partial_doubles(B, N, E, K);
  const size_t nm = (size_t)B * K * E * E;
  double *part, *mq, *aff, *off, *s0;
  int rc = carve(h->work, [&](Carver& wc) {
    part = wc.take<double>(np);
    mq = wc.take<double>(nm);
    aff = wc.take<double>((size_t)B * K * N);
    off = wc.take<double>((size_t)B * K);
    s0 = wc.take<double>((size_t)B * K);
  });
  if (rc != PBBSS_OK) return rc;
  const int f64 = o->embedding_is_f64;
  TimedRegion tr(h, s);
  if (has_model) {
    if ((rc = copy_d2d(out_mean, in_mean, (size_t)B * K * E * 8, s)) != PBBSS_OK) return rc;
    if ((rc = copy_d2d(out_covariance, in_covariance, nm * 8, s)) != PBBSS_OK) return rc;
    if ((rc = copy_d2d(out_weight, in_weight, (size_t)B * K * 8, s)) != PBBSS_OK) return rc;
    rc = pbbss::launch_gauss_full_factor(out_covariance, B * K, E, mq, off, out_status, s);
    if (rc != PBBSS_OK) return rc;
  }
  for (int it = 0; it < o->iterations; ++it) {
    const double* src = gamma0;
    if (it > 0) {  // gmm.py:129-130
      rc = pbbss::launch_gauss_full_logpdf(y, f64, B, N, E, K, out_mean, mq, off, out_weight,
                                           nullptr, aff, s);
      if (rc != PBBSS_OK) return rc;
      src = aff;
    }
    rc = pbbss::launch_gauss_full_fit(y, f64, B, N, E, K, src, saliency, part, out_mean,
                                      out_covariance, fixed_covariance ? nullptr : mq,
                                      fixed_covariance ? nullptr : off, s0, out_status, s);
    if (rc != PBBSS_OK) return rc;
    rc = pbbss::launch_gauss_full_weights(s0, B, K, o->weight_mode, out_weight, s);
    if (rc != PBBSS_OK) return rc;
    if (fixed_covariance) {  // gmm.py:160-167
      if ((rc = copy_d2d(out_covariance, fixed_covariance, nm * 8, s)) != PBBSS_OK) return rc;
      rc = pbbss::launch_gauss_full_factor(out_covariance, B * K, E, mq, off, out_status, s);
      if (rc != PBBSS_OK) return rc;
    }
  }
  if (o->final_predict && (out_affiliation || out_log_pdf)) {
    rc = pbbss::launch_gauss_full_logpdf(y, f64, B, N, E, K, out_mean, mq, off, out_weight,
                                         out_log_pdf, out_affiliation, s);
    if (rc != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}

// EM loop shared by the two real-embedding mixtures: kind = PBBSS_EMBED_VMF (rows unit-normalised
// first, vmfmm.py:76-78) or PBBSS_EMBED_GAUSS_SPHERICAL (gmm.py:126-171, covariance_type
// 'spherical'; fixed_scale = fixed_covariance (B,K) or null).
static int embed_mixture_fit(pbbss_handle_t h, int kind, const void* y, int64_t B, int64_t N, int E,
                             int K, const double* gamma0, const double* in_mean,
                             const double* in_scale, const double* in_weight,
                             const double* saliency, const double* fixed_scale,
                             const pbbss_mix_opts* o, double* out_mean, double* out_scale,
                             double* out_weight, double* out_affiliation, double* out_log_pdf,
                             void* stream) {
  if (!h || !y || !o) return PBBSS_ERR_INVALID_ARG;
  if (!embed_shape_ok(B, N, E, K)) return PBBSS_ERR_UNSUPPORTED;
  if (o->iterations < 0 || o->weight_mode < 0 || o->weight_mode > 1) return PBBSS_ERR_INVALID_ARG;
  const bool has_gamma = gamma0 != nullptr;
  const bool has_model = in_mean && in_scale && in_weight;
  if (has_gamma == has_model) return PBBSS_ERR_INVALID_ARG;
  if ((o->iterations == 0) != has_model) return PBBSS_ERR_INVALID_ARG;  // vmfmm.py:70-74
  if (!out_mean || !out_scale || !out_weight) return PBBSS_ERR_INVALID_ARG;
  const bool vmf = (kind == PBBSS_EMBED_VMF);
  hipStream_t s = as_stream(stream);
  if (K > pbbss::kEmbedMaxK) {
    // 9 ... 64 classes: one fused sweep per iteration on class tiles (embed_wide.hip), for one big
    // mixture and for many small ones alike
    void* w = h->work.grow(pbbss::embed_wide_work_doubles(B, N, E, K) * 8);
    if (!w) return PBBSS_ERR_HIP;
    int rc0;
    if (has_model) {
      if ((rc0 = copy_d2d(out_mean, in_mean, (size_t)B * K * E * 8, s)) != PBBSS_OK) return rc0;
      if ((rc0 = copy_d2d(out_scale, in_scale, (size_t)B * K * 8, s)) != PBBSS_OK) return rc0;
      if ((rc0 = copy_d2d(out_weight, in_weight, (size_t)B * K * 8, s)) != PBBSS_OK) return rc0;
    }
    TimedRegion tr(h, s);
    return pbbss::embed_wide_mixture(
        kind, y, o->embedding_is_f64, B, N, E, K, gamma0, saliency, fixed_scale, o->iterations,
        o->weight_mode, o->min_concentration, o->max_concentration, static_cast<double*>(w),
        out_mean, out_scale, out_weight, o->final_predict ? out_affiliation : nullptr,
        o->final_predict ? out_log_pdf : nullptr, h->cfg.lds_limit, s);
  }
  // many small vMF mixtures (e.g. one per frequency bin): the persistent one-workgroup-per-mixture
  // kernel runs the whole loop in ONE launch (embed.hip: vmf_bin_em_kernel); a big mixture is
  // better off spread over the chip by the sweep + finalize pair below
  if (vmf && !out_log_pdf && B >= 16) {
    const size_t lds = pbbss::vmf_bin_lds_bytes(N, E, K, o->embedding_is_f64);
    if (lds > 0 && lds <= h->cfg.lds_limit) {
      if (has_model) {
        int rc0;
        if ((rc0 = copy_d2d(out_mean, in_mean, (size_t)B * K * E * 8, s)) != PBBSS_OK) return rc0;
        if ((rc0 = copy_d2d(out_scale, in_scale, (size_t)B * K * 8, s)) != PBBSS_OK) return rc0;
        if ((rc0 = copy_d2d(out_weight, in_weight, (size_t)B * K * 8, s)) != PBBSS_OK) return rc0;
      }
      TimedRegion tr(h, s);
      const int rc2 = pbbss::launch_vmf_bin_em2(
          y, o->embedding_is_f64, B, N, E, K, o->iterations, gamma0, saliency,
          has_model ? out_mean : nullptr, has_model ? out_scale : nullptr,
          has_model ? out_weight : nullptr, o->min_concentration, o->max_concentration,
          o->weight_mode, out_mean, out_scale, out_weight,
          (o->final_predict && out_affiliation) ? out_affiliation : nullptr, h->cfg.lds_limit,
          h->cfg.num_cu > 0 ? h->cfg.num_cu : 256, s);
      if (rc2 != PBBSS_ERR_UNSUPPORTED) return rc2;
      return pbbss::launch_vmf_bin_em(
          y, o->embedding_is_f64, B, N, E, K, o->iterations, gamma0, saliency,
          has_model ? out_mean : nullptr, has_model ? out_scale : nullptr,
          has_model ? out_weight : nullptr, o->min_concentration, o->max_concentration,
          o->weight_mode, out_mean, out_scale, out_weight,
          (o->final_predict && out_affiliation) ? out_affiliation : nullptr, h->cfg.lds_limit, s);
    }
  }
  const size_t nyz = (size_t)B * N * E;
  const size_t np = pbbss::embed_partial_doubles(B, N, E, K, nullptr);
  // vMF mixture: ONE pass over the embedding per iteration (vmf_em_kernel, embed.hip) where the
  // LDS tile fits; the two-kernel path (transposed copy for the E-step, row-major sweep for the
  // M-step) otherwise, for the Gaussian mixture and for the log-pdf output
  const size_t npf = vmf ? pbbss::vmf_fused_partial_doubles(B, N, E, K, o->embedding_is_f64) : 0;
  const bool fused = npf > 0;
  const bool need_copy = !fused || (o->final_predict && out_log_pdf);
  double *yd, *rowscale, *aff, *part, *offset, *prec;
  int rc = carve(h->work, [&](Carver& wc) {
    yd = need_copy ? wc.take<double>(nyz) : nullptr;  // (B,E,N) transposed copy, INPUT type
    rowscale = need_copy ? wc.take<double>((size_t)B * N) : nullptr;  // vMF: 1 / |y_n|
    aff = fused ? nullptr : wc.take<double>((size_t)B * K * N);
    part = wc.take<double>(np > npf ? np : npf);
    offset = wc.take<double>((size_t)B * K);
    prec = wc.take<double>((size_t)B * K);
  });
  if (rc != PBBSS_OK) return rc;
  // Two-kernel path: the E-step reads the transposed copy, the M-step the caller's row-major
  // array, both in the caller's type.  The vMF mixture works on unit rows: the E-step normalises
  // its dot products itself, the M-step takes 1 / |y_n| from `rowscale`.
  const int e_f64 = o->embedding_is_f64;
  const void* fit_y = y;
  TimedRegion tr(h, s);
  if (need_copy) {
    rc = pbbss::launch_embed_prepare(y, o->embedding_is_f64, B, N, E, 0, yd, nullptr, s,
                                     vmf ? rowscale : nullptr);
    if (rc != PBBSS_OK) return rc;
  }
  if (has_model) {
    if ((rc = copy_d2d(out_mean, in_mean, (size_t)B * K * E * 8, s)) != PBBSS_OK) return rc;
    if ((rc = copy_d2d(out_scale, in_scale, (size_t)B * K * 8, s)) != PBBSS_OK) return rc;
    if ((rc = copy_d2d(out_weight, in_weight, (size_t)B * K * 8, s)) != PBBSS_OK) return rc;
  }
  for (int it = 0; it < o->iterations; ++it) {
    if (fused) {  // vmfmm.py:131-172: E-step with the previous model (or the initialisation), M-step
      rc = pbbss::launch_vmf_em(y, e_f64, B, N, E, K, it == 0 ? gamma0 : nullptr, saliency,
                                o->min_concentration, o->max_concentration, o->weight_mode, part,
                                out_mean, out_scale, out_weight, offset, prec, nullptr, 1, s);
      if (rc != PBBSS_OK) return rc;
      continue;
    }
    const double* src = gamma0;
    if (it > 0) {  // vmfmm.py:137-138 / gmm.py:129-130 (offsets: previous M-step's finalize)
      rc = pbbss::launch_embed_estep(kind, yd, e_f64, B, N, E, K, out_mean, prec, offset,
                                     out_weight, 1.0, N, nullptr, aff, s);
      if (rc != PBBSS_OK) return rc;
      src = aff;
    }
    rc = pbbss::launch_embed_fit(kind, fit_y, e_f64, B, N, E, K, src, N, saliency,
                                 o->min_concentration, o->max_concentration, o->weight_mode, part,
                                 out_mean, out_scale, out_weight, offset, prec, 0, s,
                                 vmf ? rowscale : nullptr);
    if (rc != PBBSS_OK) return rc;
    if (fixed_scale) {  // gmm.py:160-167
      if ((rc = copy_d2d(out_scale, fixed_scale, (size_t)B * K * 8, s)) != PBBSS_OK) return rc;
      rc = pbbss::launch_embed_offsets(kind, B * K, E, out_scale, offset, prec, s);
      if (rc != PBBSS_OK) return rc;
    }
  }
  if (o->final_predict && (out_affiliation || out_log_pdf)) {
    if (o->iterations == 0) {
      rc = pbbss::launch_embed_offsets(kind, B * K, E, out_scale, offset, prec, s);
      if (rc != PBBSS_OK) return rc;
    }
    if (fused && !out_log_pdf) {
      return pbbss::launch_vmf_em(y, e_f64, B, N, E, K, nullptr, nullptr, o->min_concentration,
                                  o->max_concentration, o->weight_mode, part, out_mean, out_scale,
                                  out_weight, offset, prec, out_affiliation, 0, s);
    }
    rc = pbbss::launch_embed_estep(kind, yd, e_f64, B, N, E, K, out_mean, prec, offset,
                                   out_weight, 1.0, N, out_log_pdf, out_affiliation, s);
    if (rc != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}

PBBSS_API int pbbss_vmfmm_fit(pbbss_handle_t h, const void* y, int64_t B, int64_t N, int E, int K,
                              const double* gamma0, const double* in_mean,
                              const double* in_concentration, const double* in_weight,
                              const double* saliency, const pbbss_mix_opts* o, double* out_mean,
                              double* out_concentration, double* out_weight,
                              double* out_affiliation, double* out_log_pdf, void* stream) {
  DeviceGuard device_guard(h);
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
  DeviceGuard device_guard(h);
  return embed_mixture_fit(h, PBBSS_EMBED_GAUSS_SPHERICAL, y, B, N, E, K, gamma0, in_mean,
                           in_covariance, in_weight, saliency, fixed_covariance, o, out_mean,
                           out_covariance, out_weight, out_affiliation, out_log_pdf, stream);
}

// ---------------------------------------------------------------------------
// N4: remaining beamformer family (bf_extra.hip)
// ---------------------------------------------------------------------------
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

// ---------------------------------------------------------------- STFT edge (row N4)
PBBSS_API int pbbss_stft_num_frames(int64_t num_samples, int size, int shift, int window_length,
                                    int fading, int pad) {
  if (num_samples < 0 || size < 1 || shift < 1 || window_length < 1) return PBBSS_ERR_INVALID_ARG;
  const int64_t n = num_samples + (fading ? 2 * (int64_t)(window_length - shift) : 0);
  if (n < window_length) return pad ? 1 : 0;
  const int64_t rest = n - window_length;
  const int64_t frames = 1 + (pad ? (rest + shift - 1) / shift : rest / shift);
  return frames > INT32_MAX ? PBBSS_ERR_UNSUPPORTED : (int)frames;
}

PBBSS_API int pbbss_stft(pbbss_handle_t h, const void* x, int x_is_f64, int64_t C, int64_t N,
                         int size, int shift, int window_length, const double* window, int fading,
                         int pad, int out_layout, int out_is_c128, void* out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !x || !window || !out || C <= 0 || N <= 0) return PBBSS_ERR_INVALID_ARG;
  if (fading && window_length < shift) return PBBSS_ERR_INVALID_ARG;
  const int T = pbbss_stft_num_frames(N, size, shift, window_length, fading, pad);
  if (T <= 0) return T < 0 ? T : PBBSS_ERR_INVALID_ARG;
  return pbbss::launch_stft(x, x_is_f64, C, N, size, shift, window_length, window,
                            fading ? window_length - shift : 0, T, out_layout, out_is_c128, out,
                            h->cfg.lds_limit, as_stream(stream));
}

PBBSS_API int pbbss_istft(pbbss_handle_t h, const void* X, int x_is_c128, int64_t C, int T, int size,
                          int shift, int window_length, const double* synthesis_window, int fading,
                          double* out, int64_t n_out, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !X || !synthesis_window || !out || C <= 0 || T <= 0) return PBBSS_ERR_INVALID_ARG;
  if (window_length < shift || shift < 1) return PBBSS_ERR_INVALID_ARG;
  const int fade = fading ? window_length - shift : 0;
  if (n_out != (int64_t)T * shift + window_length - shift - 2 * (int64_t)fade) return PBBSS_ERR_INVALID_ARG;
  void* wmem = h->work.grow((size_t)C * T * window_length * 8);
  if (!wmem) return PBBSS_ERR_HIP;
  return pbbss::launch_istft(X, x_is_c128, C, T, size, shift, window_length, synthesis_window, fade,
                             static_cast<double*>(wmem), out, n_out, h->cfg.lds_limit,
                             as_stream(stream));
}
