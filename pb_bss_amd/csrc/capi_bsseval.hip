// extern "C" boundary of the BSS-Eval metric (include/pbbss.h, section V5-V9; kernels:
// bss_eval.hip): argument validation and the workspace.  No device code lives here.
#include "handle.hpp"
#include "bss_eval.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

namespace {

bool aligned(const void* p, bool is_f64) {
  return reinterpret_cast<uintptr_t>(p) % (is_f64 ? 8u : 4u) == 0;
}

// PBBSS_OK and the problem, or the error code of the arguments
int make_problem(const void* reference, const void* estimation, int dtype, int64_t B, int K,
                 int Ke, int64_t N, int64_t ref_batch_stride, int64_t ref_row_stride,
                 int64_t est_batch_stride, int64_t est_row_stride, int filter_length,
                 int compute_permutation, pbbss::BssProblem* p) {
  if (dtype != PBBSS_EVAL_F32 && dtype != PBBSS_EVAL_F64) return PBBSS_ERR_INVALID_ARG;
  const bool is_f64 = dtype == PBBSS_EVAL_F64;
  if (B < 1 || K < 1 || Ke < 1 || N < 1 || filter_length < 1 || ref_batch_stride < 0 ||
      ref_row_stride < 0 || est_batch_stride < 0 || est_row_stride < 0 ||
      !aligned(reference, is_f64) || !aligned(estimation, is_f64))
    return PBBSS_ERR_INVALID_ARG;
  if (K > pbbss::kBssMaxSources || Ke > pbbss::kBssMaxSources || (Ke != K && Ke != K + 1) ||
      filter_length > pbbss::kBssMaxFilter || (!compute_permutation && Ke != K) ||
      N > (int64_t(1) << 40))
    return PBBSS_ERR_UNSUPPORTED;
  p->ref = reference;
  p->est = estimation;
  p->B = B;
  p->N = N;
  p->ref_batch = ref_batch_stride;
  p->ref_row = ref_row_stride;
  p->est_batch = est_batch_stride;
  p->est_row = est_row_stride;
  p->K = K;
  p->Ke = Ke;
  p->L = filter_length;
  p->is_f64 = is_f64;
  p->permute = compute_permutation != 0;
  return PBBSS_OK;
}

// the workspace of one group of items out of the handle's slab, and the size of the group
int carve_group(pbbss_handle_t h, const pbbss::BssProblem& p, pbbss::BssWork* w, int64_t* group) {
  *group = pbbss::bss_group_items(p);
  return pbbss::carve(h->work, [&](pbbss::Carver& c) { pbbss::bss_carve(c, p, *group, *w); });
}

}  // namespace

PBBSS_API int pbbss_bss_eval_workspace(int64_t B, int K, int Ke, int64_t N,
                                       int64_t ref_batch_stride, int filter_length,
                                       int64_t* out_bytes) {
  if (!out_bytes) return PBBSS_ERR_INVALID_ARG;
  pbbss::BssProblem p{};
  const int rc = make_problem(nullptr, nullptr, PBBSS_EVAL_F64, B, K, Ke, N, ref_batch_stride, 1,
                              1, 1, filter_length, 1, &p);
  if (rc != PBBSS_OK) return rc;
  *out_bytes = (int64_t)pbbss::bss_group_work(p, pbbss::bss_group_items(p));
  return PBBSS_OK;
}

PBBSS_API int pbbss_bss_eval(pbbss_handle_t h, const void* reference, const void* estimation,
                             int dtype, int64_t B, int K, int Ke, int64_t N,
                             int64_t ref_batch_stride, int64_t ref_row_stride,
                             int64_t est_batch_stride, int64_t est_row_stride, int filter_length,
                             int compute_permutation, double* out_sdr, double* out_sir,
                             double* out_sar, int64_t* out_selection, double* out_tables,
                             int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !reference || !estimation || !out_sdr || !out_sir || !out_sar || !out_selection ||
      !out_status)
    return PBBSS_ERR_INVALID_ARG;
  pbbss::BssProblem p{};
  const int rc = make_problem(reference, estimation, dtype, B, K, Ke, N, ref_batch_stride,
                              ref_row_stride, est_batch_stride, est_row_stride, filter_length,
                              compute_permutation, &p);
  if (rc != PBBSS_OK) return rc;
  pbbss::BssWork work{};
  int64_t group = 0;
  const int rc_work = carve_group(h, p, &work, &group);
  if (rc_work != PBBSS_OK) return rc_work;
  const pbbss::BssOutputs out{out_sdr, out_sir, out_sar, out_selection, out_tables, out_status};
  TimedRegion tr(h, as_stream(stream));
  if (h->timing)
    for (float& ms : h->bss_phase_ms) ms = 0.f;
  return pbbss::launch_bss_eval(p, nullptr, work, group, out,
                                h->timing ? h->bss_phase_ms : nullptr, as_stream(stream));
}

PBBSS_API int pbbss_bss_eval_phase_ms(pbbss_handle_t h, float* out_ms) {
  if (!h || !out_ms) return PBBSS_ERR_INVALID_ARG;
  for (int i = 0; i < 4; ++i) out_ms[i] = h->bss_phase_ms[i];
  return PBBSS_OK;
}

PBBSS_API int pbbss_bss_eval_system(pbbss_handle_t h, const void* reference,
                                    const void* estimation, int dtype, int64_t B, int K, int Ke,
                                    int64_t N, int64_t ref_batch_stride, int64_t ref_row_stride,
                                    int64_t est_batch_stride, int64_t est_row_stride,
                                    int filter_length, double* out_gram, double* out_rhs,
                                    void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !reference || !estimation || !out_gram || !out_rhs) return PBBSS_ERR_INVALID_ARG;
  pbbss::BssProblem p{};
  const int rc = make_problem(reference, estimation, dtype, B, K, Ke, N, ref_batch_stride,
                              ref_row_stride, est_batch_stride, est_row_stride, filter_length, 1,
                              &p);
  if (rc != PBBSS_OK) return rc;
  pbbss::BssWork work{};
  int64_t group = 0;
  const int rc_work = carve_group(h, p, &work, &group);
  if (rc_work != PBBSS_OK) return rc_work;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_bss_system(p, work, group, out_gram, out_rhs, as_stream(stream));
}

PBBSS_API int pbbss_bss_eval_filters(pbbss_handle_t h, const void* reference,
                                     const void* estimation, int dtype, int64_t B, int K, int Ke,
                                     int64_t N, int64_t ref_batch_stride, int64_t ref_row_stride,
                                     int64_t est_batch_stride, int64_t est_row_stride,
                                     int filter_length, int compute_permutation,
                                     const double* filters_all, const double* filters_single,
                                     double* out_sdr, double* out_sir, double* out_sar,
                                     int64_t* out_selection, double* out_tables,
                                     int32_t* out_status, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !reference || !estimation || !filters_all || !filters_single || !out_sdr ||
      !out_sir || !out_sar || !out_selection || !out_status)
    return PBBSS_ERR_INVALID_ARG;
  pbbss::BssProblem p{};
  const int rc = make_problem(reference, estimation, dtype, B, K, Ke, N, ref_batch_stride,
                              ref_row_stride, est_batch_stride, est_row_stride, filter_length,
                              compute_permutation, &p);
  if (rc != PBBSS_OK) return rc;
  pbbss::BssWork work{};
  int64_t group = 0;
  const int rc_work = carve_group(h, p, &work, &group);
  if (rc_work != PBBSS_OK) return rc_work;
  const pbbss::BssFilters filters{filters_all, filters_single};
  const pbbss::BssOutputs out{out_sdr, out_sir, out_sar, out_selection, out_tables, out_status};
  TimedRegion tr(h, as_stream(stream));
  return pbbss::launch_bss_eval(p, &filters, work, group, out, nullptr, as_stream(stream));
}
