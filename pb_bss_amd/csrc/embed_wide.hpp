// Real-embedding mixtures with MANY classes (9 <= K <= 64): von Mises-Fisher, spherical and
// diagonal Gaussians on FP64 matrix-pipe tiles.  Host-side launchers; kernels live in
// embed_wide.hip.  embed.hip keeps one accumulator per class and lane (K <= kEmbedMaxK); here a
// row's classes lie across the 16 lanes of a DPP row and up to four class tiles, so that both
// contractions of an EM iteration -- (N x E)(E x K) for the class log-pdfs, (K x N)(N x E) for the
// weighted sums -- fill v_mfma_f64_16x16x4_f64 tiles.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "pbbss.h"
#include "embed.hpp"

namespace pbbss {

constexpr int kEmbedWideMaxK = 64;  // four class tiles of 16

// doubles of workspace any of the three calls below needs for the shape (chunk partials of both
// moment sets, the padded sweep model, per-class weight sums, the common shift)
size_t embed_wide_work_doubles(int64_t B, int64_t N, int E, int K);

// The EM loop of pbbss_vmfmm_fit / pbbss_gmm_fit (run_embed_mixture_fit in embed_fit.hip) for K > 8: per
// iteration ONE sweep over the caller's row-major y (wide_sweep_kernel: E-step tile, softmax
// across the DPP row, M-step tiles from the same LDS rows) + the ordered finalize + the model
// kernel that prepares the next sweep.  Arguments as embed_mixture_fit; fixed_scale (B, K) or
// null; the model of an iterations == 0 call is already in out_mean / out_scale / out_weight.
int embed_wide_mixture(int kind, const void* y, int y_is_f64, int64_t B, int64_t N, int E, int K,
                       const double* gamma0, const double* saliency, const double* fixed_scale,
                       int iterations, int weight_mode, double cmin, double cmax, double* work,
                       double* out_mean, double* out_scale, double* out_weight, double* out_aff,
                       double* out_lp, size_t lds_limit, hipStream_t s);

// pbbss_embed_fit for K > 8: w_k(n) = weights[index(b, k, n)] * (sal ? sal[b N + n] : 1) with the
// index of launch_embed_estep (Tin = N: plain (B, K, N); Tin = T: the (F, K, T) affiliations of
// the joint models); vMF: rows scaled to unit norm on the fly when `normalize`; Gaussians: both
// moments about a common shift in one sweep ('diagonal': a second sweep over the squares).
int embed_wide_fit(int kind, const void* y, int y_is_f64, int64_t B, int64_t N, int E, int K,
                   const double* weights, int normalize, double cmin, double cmax, double* work,
                   double* out_mean, double* out_scale, size_t lds_limit, hipStream_t s,
                   int64_t Tin = 0, const double* sal = nullptr, bool have_shift = false);

// class log-pdfs (times out_scale) of every sample for K > 8; out index as launch_embed_estep
// (Tin = N: plain (B, K, N); Tin = T: 'k,ft->fkt').  PBBSS_EMBED_GAUSS_DIAG (B = 1): the
// reference's formula (see embed.hip), u_j = pc_j . y as one tile set, the cross term as a second.
int embed_wide_log_pdf(int kind, const void* y, int y_is_f64, int64_t B, int64_t N, int E, int K,
                       const double* mean, const double* scale, double out_scale, int64_t Tin,
                       double* work, double* out_lp, size_t lds_limit, hipStream_t s,
                       bool have_shift = false);

// The Gaussians' common shift (column mean of every mixture) into `work`, once per fit: a loop that
// calls embed_wide_fit / embed_wide_log_pdf on the SAME y and work passes have_shift = true.
int embed_wide_shift(int kind, const void* y, int y_is_f64, int64_t B, int64_t N, int E, int K,
                     double* work, hipStream_t s);

// launch_joint_weight (embed.hpp) for K > 8: same modes, same scratch (joint_weight_tmp_doubles)
int embed_wide_joint_weight(int mode, const double* aff, const double* sal, int64_t F, int K, int T,
                            double* tmp, double* out_weight, hipStream_t s);

}  // namespace pbbss
