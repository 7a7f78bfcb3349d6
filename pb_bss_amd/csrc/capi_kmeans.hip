// extern "C" boundary of k-means (include/pbbss.h, section W; kernels: kmeans.hip): argument
// validation and the workspaces.  No device code lives here.
#include <algorithm>
#include "handle.hpp"
#include "kmeans.hpp"

using pbbss::as_stream, pbbss::DeviceGuard, pbbss::TimedRegion;

static bool kmeans_aligned(const void* p, int is_f64) {
  return reinterpret_cast<uintptr_t>(p) % (is_f64 ? 8u : 4u) == 0;
}

static int kmeans_work(pbbss_handle_t h, const pbbss::KmeansGeom& g, pbbss::KmeansWork* w) {
  // the tolerance pass writes (E + 1)-long partials into the same place as the sweeps
  const size_t P = std::max<size_t>(pbbss::kmeans_part_len(g), (size_t)g.E + 1);
  return pbbss::carve(h->work, [&](pbbss::Carver& c) {
    w->part = c.take<double>((size_t)g.B * g.C * P);
    w->tot = c.take<double>((size_t)g.B * g.K * (g.E + 1));
    w->mind = c.take<double>((size_t)g.B * g.N);
    w->mean = c.take<double>((size_t)g.B * (g.E + 1));
    w->tol_abs = c.take<double>((size_t)g.B);
    w->state = c.take<int32_t>((size_t)g.B);
    w->flags = c.take<int32_t>(2);
  });
}

PBBSS_API int pbbss_kmeans_fit(pbbss_handle_t h, const void* y, int y_is_f64, int64_t B, int64_t N,
                               int E, int K, const uint8_t* saliency, const double* in_centers,
                               int max_iter, double tol, int block, double* out_centers,
                               int32_t* out_labels, double* out_inertia, int32_t* out_n_iter,
                               void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !in_centers || !out_centers || !out_labels || !out_inertia || !out_n_iter ||
      B < 1 || N < 1 || E < 1 || K < 1 || max_iter < 1 || block < 1 || !(tol >= 0.0) ||
      !kmeans_aligned(y, y_is_f64))
    return PBBSS_ERR_INVALID_ARG;
  if (K > N) return PBBSS_ERR_INVALID_ARG;  // as sklearn: n_samples should be >= n_clusters
  pbbss::KmeansGeom g{};
  if (!pbbss::kmeans_geom(B, N, E, K, y_is_f64 != 0, &g)) return PBBSS_ERR_UNSUPPORTED;
  pbbss::KmeansWork w{};
  int rc = kmeans_work(h, g, &w);
  if (rc != PBBSS_OK) return rc;
  hipStream_t s = as_stream(stream);
  TimedRegion tr(h, s);
  rc = pbbss::copy_d2d(out_centers, in_centers, (size_t)B * K * E * sizeof(double), s);
  if (rc != PBBSS_OK) return rc;
  return pbbss::run_kmeans_fit(g, w, y, saliency, max_iter, tol, block, out_centers, out_labels,
                               out_inertia, out_n_iter, s);
}

PBBSS_API int pbbss_kmeans_predict(pbbss_handle_t h, const void* y, int y_is_f64, int64_t B,
                                   int64_t N, int E, int K, const double* centers,
                                   int32_t* out_labels, void* out_one_hot, double* out_inertia,
                                   void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !centers || !out_labels || B < 1 || N < 1 || E < 1 || K < 1 ||
      !kmeans_aligned(y, y_is_f64) || !kmeans_aligned(out_one_hot, y_is_f64))
    return PBBSS_ERR_INVALID_ARG;
  pbbss::KmeansGeom g{};
  if (!pbbss::kmeans_geom(B, N, E, K, y_is_f64 != 0, &g)) return PBBSS_ERR_UNSUPPORTED;
  pbbss::KmeansWork w{};
  const int rc = pbbss::carve(h->work, [&](pbbss::Carver& c) {
    w.part = c.take<double>((size_t)g.B * g.C * pbbss::kmeans_part_len(g));
    w.state = c.take<int32_t>((size_t)g.B);
  });
  if (rc != PBBSS_OK) return rc;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::run_kmeans_predict(g, w, y, centers, out_labels, out_one_hot, out_inertia,
                                   as_stream(stream));
}

PBBSS_API int pbbss_kmeans_plusplus(pbbss_handle_t h, const void* y, int y_is_f64, int64_t B,
                                    int64_t N, int E, int K, const uint8_t* saliency, int trials,
                                    const double* randoms, int32_t* out_indices,
                                    double* out_centers, void* stream) {
  DeviceGuard device_guard(h);
  if (!h || !y || !randoms || !out_indices || !out_centers || B < 1 || N < 1 || E < 1 || K < 1 ||
      trials < 1 || !kmeans_aligned(y, y_is_f64))
    return PBBSS_ERR_INVALID_ARG;
  if (K > N) return PBBSS_ERR_INVALID_ARG;
  pbbss::KmeansGeom g{};
  if (trials > pbbss::kKmeansMaxTrials || !pbbss::kmeans_geom(B, N, E, K, y_is_f64 != 0, &g))
    return PBBSS_ERR_UNSUPPORTED;
  pbbss::KmeansSeedWork w{};
  const int rc = pbbss::carve(h->work, [&](pbbss::Carver& c) {
    w.closest = c.take<double>((size_t)g.B * g.N);
    w.csum = c.take<double>((size_t)g.B * g.scan_chunks);
    w.cpart = c.take<double>((size_t)g.B * g.scan_chunks * pbbss::kKmeansMaxTrials);
    w.cand = c.take<int32_t>((size_t)g.B * pbbss::kKmeansMaxTrials);
    w.chosen = c.take<int32_t>((size_t)g.B);
  });
  if (rc != PBBSS_OK) return rc;
  TimedRegion tr(h, as_stream(stream));
  return pbbss::run_kmeans_plusplus(g, w, y, saliency, trials, randoms, out_indices, out_centers,
                                    as_stream(stream));
}
