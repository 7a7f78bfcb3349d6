// Persistent complex-Bingham mixture-model (cBMM) EM kernel for gfx950, and the Bingham
// parameter solve on its own.
//
// Reference: distribution/cbmm.py:21-58 (CBMM.predict / _predict), :205-237 (_fit / _m_step),
// distribution/complex_bingham.py:38-79 (covariance, log_pdf), :84-186 (norm), :188-224
// (_remove_duplicate_eigenvalues), :304-396 (find_eigenvalues_v3), :571-594 (_fit).
//
// Same skeleton as the Watson kernel (cwmm.hpp): frames LDS-resident, one bin per workgroup,
//   E  q_kt = <B_k, P_t> (the full Hermitian quadratic form of cacgmm_em.hpp, a linear link):
//      log p = q_kt - ln c(lam_k); softmax with a max-shift, weights in the linear domain
//   M  C_k = sum_t gamma_kt P_t / sum_t gamma_kt      (Watson's plain weighted scatter)
//   F  wave k: Jacobi eigendecomposition of C_k -> scatter eigenvalues s (ascending), V;
//      de-duplication; the bounded Gauss-Newton solve for lam (below); the max_concentration
//      clamp and a second de-duplication; B_k = V diag(lam) V^H and ln c of the de-duplicated lam.
//
// Normaliser.  c(lam) = 2 pi^D e[lam_1..lam_D], the divided difference of exp.  The reference's
// partial-fraction form loses ~8 digits per near-equal pair; here e[.] is the top-right entry of
// the exponential of the bidiagonal matrix (nodes on the diagonal, ones above), by scaling and
// squaring: the nodes are shifted by the largest one, scaled by 2^-s to a width <= 1, each entry
// of the scaled exponential is a 16-term Taylor series in the complete homogeneous symmetric
// polynomials of the (centred) nodes, and s squarings of the upper-triangular table follow.
// Every entry is positive, so the squarings add positive terms only (no cancellation at any node
// spacing).  Derivatives duplicate nodes:
//   g_i = e[lam, lam_i] / e[lam],   H_ij = (1 + d_ij) e[lam, lam_i, lam_j] / e[lam] - g_i g_j,
// one (D+2)-node table per lane, lane p <-> pair (i <= j).
//
// Solve.  Unknowns: the D-1 consecutive differences delta_j = lam_j - lam_{j+1} of the sorted lam
// (lam_{D-1} = 0), boxed to [-max_concentration, -1e-8]; residual r = g(lam) - s (D components),
// Jacobian J = H U (U: d lam / d delta).  Projected Gauss-Newton with an active set (a variable at
// a bound whose gradient component points outwards is held), the step by modified Gram-Schmidt
// (twice) on the free columns, backtracking on |r|^2.  Without an active bound this is Newton on
// the root.  Start x0 = -1/s as the reference; stop when rho = max |Q^T r| (the part of r the free
// unknowns can still change) is <= 1e-15, or when it stops falling (its rounding floor, which
// rises as the smallest scatter eigenvalue falls: ~1e-12 at 1e-6), or when no step along the
// Gauss-Newton direction descends.  PBBSS_ST_SOLVE_NOCONV: the iteration cap reached while still
// progressing, or a stationary point with rho > 1e-6.
#pragma once
#include "cacgmm_em.hpp"

namespace pbbss {

constexpr int kBinghamTaylor = 16;
constexpr int kBinghamMaxIter = 100;
constexpr int kBinghamMaxHalvings = 8;
constexpr double kBinghamTol = 1e-15;      // rho target
constexpr double kBinghamAccept = 1e-13;   // rho below which a stall ends the solve at once
constexpr double kBinghamStallRatio = 0.9;  // a step that keeps >= 90 % of rho gains nothing ...
constexpr int kBinghamStallSteps = 3;       // ... and three of them in a row mark the floor
constexpr double kBinghamGross = 1e-6;     // rho above which a stationary point is a failure
constexpr double kBinghamDeltaMax = -1e-8;  // complex_bingham.py:376

struct BinghamArgs {
  EmArgs em;                 // y, B, T, gamma0, saliency, iterations, weight_mode, outputs
  const double* in_eigvec;   // c128 (B,K,D,D) or null
  const double* in_eigval;   // (B,K,D)
  double max_concentration;  // +inf: no clamp
  double eigenvalue_eps;
  double norm_eps;           // de-duplication spacing of ln c (ComplexBingham.norm's eps, 1e-8)
  double* out_eigvec;        // c128 (B,K,D,D), eigh order
  double* out_eigval;        // (B,K,D)
  double* out_lognorm;       // (B,K)
};

// 1 / k! for the Taylor sums (k <= kBinghamTaylor + 9)
__device__ __forceinline__ constexpr double bingham_invfact(int k) {
  double f = 1.0;
  for (int i = 2; i <= k; ++i) f *= (double)i;
  return 1.0 / f;
}

// e[x_a..x_b] * exp(-shift) for a <= b in A (per lane, N nodes in registers).
template <int N>
__device__ __forceinline__ void exp_dd_table(const double (&x)[N], double (&A)[N][N],
                                             double& shift) {
  double c = x[0], lo = x[0];
#pragma unroll
  for (int i = 1; i < N; ++i) {
    c = fmax(c, x[i]);
    lo = fmin(lo, x[i]);
  }
  const double r = c - lo;
  int s = 0;
  if (r > 1.0) {
    int e;
    const double m = frexp(r, &e);
    s = (m == 0.5) ? e - 1 : e;  // ceil(log2 r)
    s = min(s, 1100);
  }
  const double scale = ldexp(1.0, -s);
  const double cy = -0.5 * r * scale;
  const double ecy = exp(cy);
  double y[N];
#pragma unroll
  for (int i = 0; i < N; ++i) y[i] = (x[i] - c) * scale - cy;
  double pw[N];
  pw[0] = ecy;
#pragma unroll
  for (int m = 1; m < N; ++m) pw[m] = pw[m - 1] * scale;
#pragma unroll
  for (int a = 0; a < N; ++a) {
    double h[kBinghamTaylor + 1];
    h[0] = 1.0;
#pragma unroll
    for (int k = 1; k <= kBinghamTaylor; ++k) h[k] = 0.0;
#pragma unroll
    for (int b = a; b < N; ++b) {
      const double z = y[b];
#pragma unroll
      for (int k = 1; k <= kBinghamTaylor; ++k) h[k] = fma(z, h[k - 1], h[k]);
      const int m = b - a;
      double tot = 0.0;
#pragma unroll
      for (int k = kBinghamTaylor; k >= 0; --k) tot = fma(h[k], bingham_invfact(k + m), tot);
      A[a][b] = tot * pw[m];
    }
  }
  // squarings, in place: row a ascending, column b descending (reads only entries not yet
  // overwritten: A[a][k] for k <= b and rows below a)
  for (int it = 0; it < s; ++it) {
#pragma unroll
    for (int a = 0; a < N; ++a) {
#pragma unroll
      for (int b = N - 1; b >= a; --b) {
        double acc = 0.0;
#pragma unroll
        for (int k = a; k <= b; ++k) acc = fma(A[a][k], A[k][b], acc);
        A[a][b] = acc;
      }
    }
  }
  shift = c;
}

// wave-uniform array element by a per-lane index
template <int D>
__device__ __forceinline__ double sel(const double (&v)[D], int i) {
  double r = v[0];
#pragma unroll
  for (int m = 1; m < D; ++m) r = (i == m) ? v[m] : r;
  return r;
}

__host__ __device__ constexpr int bingham_pair_lane(int D, int i, int j) {
  return i * D - (i * (i - 1)) / 2 + (j - i);
}

// ln e[lam] (any order; wave-uniform result)
template <int D>
__device__ __forceinline__ double bingham_log_e(const double (&lam)[D]) {
  double A[D][D], c;
  exp_dd_table<D>(lam, A, c);
  return c + log(A[0][D - 1]);
}

// ln c(lam) = ln(2 pi^D e[lam]) (complex_bingham.py:180-186)
template <int D>
__device__ __forceinline__ double bingham_log_norm_sorted(const double (&lam)[D]) {
  return 0.6931471805599453 + (double)D * 1.1447298858494002 + bingham_log_e<D>(lam);
}

// g and H at lam (wave-uniform in and out); every lane of the wave takes part
template <int D>
__device__ void bingham_grad_hess(const double (&lam)[D], int lane, double (&g)[D],
                                  double (&H)[D][D]) {
  constexpr int N = D + 2;
  constexpr int NP = D * (D + 1) / 2;
  static_assert(NP <= kWave, "one pair per lane");
  int ip = 0, jp = 0;  // lanes >= NP: a copy of pair (0, 0)
#pragma unroll
  for (int i = 0; i < D; ++i) {
#pragma unroll
    for (int j = i; j < D; ++j) {
      if (lane == bingham_pair_lane(D, i, j)) {
        ip = i;
        jp = j;
      }
    }
  }
  double x[N];
#pragma unroll
  for (int i = 0; i < D; ++i) x[i] = lam[i];
  x[D] = sel<D>(lam, ip);
  x[D + 1] = sel<D>(lam, jp);
  double A[N][N], c;
  exp_dd_table<N>(x, A, c);
  const double r0 = 1.0 / A[0][D - 1];
  const double e1 = A[0][D] * r0, e2 = A[0][D + 1] * r0;
#pragma unroll
  for (int i = 0; i < D; ++i) g[i] = lane_bcast_const(e1, bingham_pair_lane(D, i, i));
#pragma unroll
  for (int i = 0; i < D; ++i) {
#pragma unroll
    for (int j = i; j < D; ++j) {
      const double v = (i == j ? 2.0 : 1.0) * lane_bcast_const(e2, bingham_pair_lane(D, i, j)) -
                       g[i] * g[j];
      H[i][j] = v;
      H[j][i] = v;
    }
  }
}

// _remove_duplicate_eigenvalues on an ascending array (complex_bingham.py:215-221)
template <int D>
__device__ __forceinline__ void bingham_dedup(double (&v)[D], double eps) {
  const double v0 = v[0];
  double acc = 0.0, prev = v[0];
#pragma unroll
  for (int i = 1; i < D; ++i) {
    const double cur = v[i];
    acc += fmax(cur - prev, eps);
    prev = cur;
    v[i] = v0 + acc;
  }
}

template <int D>
__device__ __forceinline__ void bingham_lam_of(const double (&delta)[D - 1], double (&lam)[D]) {
  lam[D - 1] = 0.0;
  double acc = 0.0;
#pragma unroll
  for (int i = D - 2; i >= 0; --i) {
    acc += delta[i];
    lam[i] = acc;
  }
}

// residual r = g(lam(delta)) - s and H; returns |r|^2
template <int D>
__device__ __forceinline__ double bingham_residual(const double (&delta)[D - 1],
                                                   const double (&s)[D], int lane,
                                                   double (&r)[D], double (&H)[D][D]) {
  double lam[D], g[D];
  bingham_lam_of<D>(delta, lam);
  bingham_grad_hess<D>(lam, lane, g, H);
  double f = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    r[i] = g[i] - s[i];
    f = fma(r[i], r[i], f);
  }
  return f;
}

// Gauss-Newton step on the free columns of J (modified Gram-Schmidt, twice); -> rho
template <int D>
__device__ __forceinline__ double bingham_gn_step(const double (&H)[D][D], const double (&r)[D],
                                                  const bool (&fr)[D - 1],
                                                  double (&step)[D - 1]) {
  constexpr int M = D - 1;
  double Q[M][D], R[M][M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    // column j of J = H U: sum of the first j+1 columns of H
#pragma unroll
    for (int d = 0; d < D; ++d) {
      double v = 0.0;
#pragma unroll
      for (int i = 0; i <= j; ++i) v += H[d][i];
      Q[j][d] = fr[j] ? v : 0.0;
    }
#pragma unroll
    for (int i = 0; i < M; ++i) R[i][j] = 0.0;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int i = 0; i < j; ++i) {
        double pr = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) pr = fma(Q[i][d], Q[j][d], pr);
        R[i][j] += pr;
#pragma unroll
        for (int d = 0; d < D; ++d) Q[j][d] = fma(-pr, Q[i][d], Q[j][d]);
      }
    }
    double n2 = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) n2 = fma(Q[j][d], Q[j][d], n2);
    const double nrm = sqrt(n2);
    const bool ok = fr[j] && nrm > 0.0;
    const double inv = ok ? 1.0 / nrm : 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) Q[j][d] *= inv;
    R[j][j] = ok ? nrm : 1.0;
#pragma unroll
    for (int i = 0; i < j; ++i) R[i][j] = ok ? R[i][j] : 0.0;
  }
  double qtr[M], rho = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double v = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) v = fma(Q[j][d], r[d], v);
    qtr[j] = v;
    rho = fmax(rho, fabs(v));
  }
#pragma unroll
  for (int j = M - 1; j >= 0; --j) {
    double acc = -qtr[j];
#pragma unroll
    for (int k = j + 1; k < M; ++k) acc = fma(-R[j][k], step[k], acc);
    step[j] = acc / R[j][j];
  }
  return rho;
}

// find_eigenvalues_v3 for ascending scatter eigenvalues s (wave-uniform; every lane of the wave
// calls it) -> ascending lam after the clamp and the second de-duplication.  Returns status bits.
template <int D>
__device__ int bingham_find_eigenvalues(const double (&s_in)[D], double eps, double maxc,
                                        int lane, double (&lam)[D]) {
  constexpr int M = D - 1;
  int st = 0;
  double s[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    s[i] = s_in[i];
    if (!isfinite(s[i]) || s[i] < 0.0) st |= PBBSS_ST_NONFINITE;  // complex_bingham.py:589
  }
  bingham_dedup<D>(s, eps);
  const double lo = -maxc, hi = kBinghamDeltaMax;
  double x0[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    x0[i] = (i == D - 1) ? 0.0 : -1.0 / s[i];
    if (isfinite(maxc)) x0[i] = fmax(x0[i], -(maxc - (double)i));
  }
  double delta[M];
#pragma unroll
  for (int j = 0; j < M; ++j) delta[j] = fmin(fmax(x0[j] - x0[j + 1], lo), hi);
  double r[D], H[D][D];
  double f = bingham_residual<D>(delta, s, lane, r, H);
  double rho = 1e300, rho_prev = 1e300;
  bool settled = false;  // stopped at the solution or at its rounding floor (not by the cap)
  int stall = 0;
  for (int it = 0; it < kBinghamMaxIter; ++it) {
    bool fr[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double Gj = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        double Jdj = 0.0;
#pragma unroll
        for (int i = 0; i <= j; ++i) Jdj += H[d][i];
        Gj = fma(Jdj, r[d], Gj);
      }
      fr[j] = !((delta[j] <= lo && Gj > 0.0) || (delta[j] >= hi && Gj < 0.0));
    }
    double step[M];
    rho = bingham_gn_step<D>(H, r, fr, step);
    if (!(rho > kBinghamTol)) {  // NaN: reported below
      settled = (rho == rho);
      break;
    }
    // the floor: how far rho can fall depends on the conditioning of J (a scatter eigenvalue of
    // 1e-6 leaves it near 1e-12), so the stop is tied to progress, not to an absolute bound --
    // a quick exit once rho is at 1e-13 and stops halving, or three steps that gain < 10 %
    stall = (rho >= kBinghamStallRatio * rho_prev) ? stall + 1 : 0;
    if ((rho <= kBinghamAccept && rho >= 0.5 * rho_prev) || stall >= kBinghamStallSteps) {
      settled = true;
      break;
    }
    rho_prev = rho;
    double alpha = 1.0;
    bool accepted = false;
    for (int h = 0; h < kBinghamMaxHalvings && !accepted; ++h) {
      double cand[M], rc[D], Hc[D][D];
#pragma unroll
      for (int j = 0; j < M; ++j) cand[j] = fmin(fmax(fma(alpha, step[j], delta[j]), lo), hi);
      const double fc = bingham_residual<D>(cand, s, lane, rc, Hc);
      if (fc <= f * (1.0 + 1e-12) + 1e-300) {
        accepted = true;
        f = fc;
#pragma unroll
        for (int j = 0; j < M; ++j) delta[j] = cand[j];
#pragma unroll
        for (int i = 0; i < D; ++i) {
          r[i] = rc[i];
#pragma unroll
          for (int j = 0; j < D; ++j) H[i][j] = Hc[i][j];
        }
      } else {
        alpha *= 0.5;
      }
    }
    if (!accepted) {  // no descent along the Gauss-Newton step: stationary within rounding
      settled = true;
      break;
    }
  }
  // not converged: the iteration cap while still making progress, or a stationary point whose
  // rho is far above any rounding floor (a rank-deficient J)
  if (!settled || !(rho <= kBinghamGross)) st |= PBBSS_ST_SOLVE_NOCONV;
  bingham_lam_of<D>(delta, lam);
  if (isfinite(maxc)) {  // complex_bingham.py:391-396
#pragma unroll
    for (int i = 0; i < D; ++i) lam[i] = fmax(lam[i], -maxc);
    bingham_dedup<D>(lam, eps);
  }
#pragma unroll
  for (int i = 0; i < D; ++i)
    if (!isfinite(lam[i])) st |= PBBSS_ST_NONFINITE;
  return st;
}

// SPILL: observation, norms and M-step weights in a per-workgroup HBM scratch slab (utterances
// whose frames exceed the LDS), as the cACGMM and Watson kernels do
template <int D, int K, typename YS, bool SPILL>
struct BinghamKernel {
  using Base = EmKernel<D, K, YS, SPILL>;
  using Lds = typename Base::Lds;
  static constexpr int NA = Base::NA;
  static constexpr int NOFF = Base::NOFF;
  // L.apack[k] holds B_k (dot-ready, cacgmm_em.hpp: store_apack), L.rdet[k] holds ln c(lam_k)

  // <B_k, P_t> unscaled (cacgmm_em.hpp: quad_forms without the |.| and floor of the cACG link)
  static __device__ __forceinline__ void forms(const Lds& L, const double (&re)[D],
                                               const double (&im)[D], double (&q)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = 0.0;
    static_for<0, D>([&](auto ic) {
      constexpr int i = ic;
      const double dg = re[i] * re[i] + im[i] * im[i];
#pragma unroll
      for (int k = 0; k < K; ++k) q[k] = fma(L.apack[k * NA + i], dg, q[k]);
    });
    static_for<0, NOFF>([&](auto pc) {
      constexpr int p = pc;
      constexpr int i = tri_i<D>(p), j = tri_j<D>(p);
      const double pr = re[i] * re[j] + im[i] * im[j];
      const double pim = im[i] * re[j] - re[i] * im[j];
#pragma unroll
      for (int k = 0; k < K; ++k)
        q[k] = fma(L.apack[k * NA + D + 2 * p], pr, fma(L.apack[k * NA + D + 2 * p + 1], pim, q[k]));
    });
  }

  template <bool FINAL>
  static __device__ void phase_e(const BinghamArgs& ba, const Lds& L, int64_t b, int tid,
                                 int wave, int lane) {
    const EmArgs& a = ba.em;
    double s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (int t0 = 0; t0 < a.T; t0 += kEmThreads) {
      if (t0 + wave * kWave >= Base::padded_frames(a.T)) break;
      const int tt = t0 + tid;
      const bool ok = tt < a.T;
      const int t = ok ? tt : a.T - 1;
      double re[D], im[D], q[K];
      Base::load_frame(L, tt, re, im);
      forms(L, re, im, q);
      const double inv = L.inv_n2[tt];
      double lp[K], mx = -1.79e308;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        lp[k] = q[k] * inv - L.rdet[k];  // complex_bingham.py:73-77
        mx = fmax(mx, lp[k]);
      }
      double g[K], den = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        g[k] = exp_nonpos(lp[k] - mx) * L.wgt[k];  // mixture_model_utils.py:32-37
        den += g[k];
      }
      const double rden = fast_rcp(fmax(den, kTiny)) + (den - den);
      const double sal = (!FINAL && a.saliency) ? a.saliency[(size_t)b * a.T + t] : 1.0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double gam = g[k] * rden;
        if constexpr (FINAL) {
          if (ok) {
            const size_t idx = ((size_t)b * K + k) * a.T + t;
            if (a.out_aff) a.out_aff[idx] = gam;
            if (a.out_logpdf) a.out_logpdf[idx] = lp[k];
          }
        } else {
          const double gs = ok ? gam * sal : 0.0;
          L.wbuf[Base::woff(k, tt)] = gs * inv;  // complex_bingham.py:577-580
          s[k] += gs;
        }
      }
    }
    if constexpr (!FINAL) wave_class_sums<K>(s, lane, L.red + wave * K);
  }

  // affiliation initialisation -> M-step weights (cbmm.py:221-233 with saliency)
  static __device__ void phase_init_gamma(const EmArgs& a, const Lds& L, int64_t b, int tid,
                                          int wave, int lane) {
    double s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (int t = tid; t < a.T; t += kEmThreads) {
      const double sal = a.saliency ? a.saliency[(size_t)b * a.T + t] : 1.0;
      const double inv = L.inv_n2[t];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double g = a.gamma0[((size_t)b * K + k) * a.T + t] * sal;
        L.wbuf[Base::woff(k, t)] = g * inv;
        s[k] += g;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double tot = wave_sum(s[k]);
      if (lane == 0) L.red[wave * K + k] = tot;
    }
  }

  // B = V diag(lam) V^H on lanes (i, j); lam_col: lam of this lane's column
  static __device__ __forceinline__ void cov_from_eig(double vre, double vim, double lam_col,
                                                      LaneIJ c, double& gre, double& gim) {
    gre = 0.0;
    gim = 0.0;
#pragma unroll
    for (int e = 0; e < D; ++e) {
      const double l = lane_get(lam_col, ij_lane(0, e));
      const double ar = lane_get(vre, ij_lane(c.i, e)), ai = lane_get(vim, ij_lane(c.i, e));
      const double br = lane_get(vre, ij_lane(c.j, e)), bi = lane_get(vim, ij_lane(c.j, e));
      gre += (ar * br + ai * bi) * l;
      gim += (ai * br - ar * bi) * l;
    }
  }

  // sorted (ascending, ties by column) values of the columns: rank of this lane's column and
  // the wave-uniform sorted array
  static __device__ __forceinline__ void sort_columns(double lam_col, LaneIJ c, int& rank,
                                                      double (&srt)[D]) {
    rank = wave_sort_rank<D>(lam_col, c);
#pragma unroll
    for (int r = 0; r < D; ++r) srt[r] = 0.0;
#pragma unroll
    for (int m = 0; m < D; ++m) {
      const double lm = lane_get(lam_col, ij_lane(0, m));
      const int rm = lane_get(rank, ij_lane(0, m));
#pragma unroll
      for (int r = 0; r < D; ++r) srt[r] = (rm == r) ? lm : srt[r];
    }
  }

  // ln c of the model's lam (ComplexBingham.log_norm: its own de-duplication at 1e-8)
  static __device__ __forceinline__ double log_norm_of(const double (&srt)[D], double eps) {
    double v[D];
#pragma unroll
    for (int i = 0; i < D; ++i) v[i] = srt[i];
    bingham_dedup<D>(v, eps);
    return bingham_log_norm_sorted<D>(v);
  }

  static __device__ void factor_class(const BinghamArgs& ba, const Lds& L, int64_t b, int k,
                                      int lane, bool last) {
    const EmArgs& a = ba.em;
    lane = opaque(lane);
    const LaneIJ c = lane_ij(lane);
    const bool valid = c.i < D && c.j < D;
    double are = 0.0, aim = 0.0;
    if (valid) Base::cov_entry(L, k, c.i, c.j, are, aim);
    double S = 0.0, tot = 0.0;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
      double sk = 0.0;
#pragma unroll
      for (int w = 0; w < kEmWaves; ++w) sk += L.red[w * K + kk];
      tot += fabs(sk);
      S = (kk == k) ? sk : S;
    }
    if (valid) {  // complex_bingham.py:582 (no floor in the reference)
      are /= S;
      aim /= S;
    }
    int st = 0;
    if (wave_or((isfinite(are) && isfinite(aim)) ? 0 : 1)) st |= PBBSS_ST_NONFINITE;
    double vre, vim;
    const int sweeps = wave_jacobi_heev<D>(are, aim, c, vre, vim);
    if (sweeps < 0) st |= PBBSS_ST_EIG_NOCONV;
    const double ev = lane_get(are, ij_lane(c.j, c.j));  // eigenvalue of this lane's column
    int rank;
    double s[D];
    sort_columns(ev, c, rank, s);
    double lam[D];
    st |= bingham_find_eigenvalues<D>(s, ba.eigenvalue_eps, ba.max_concentration, lane, lam);
    const double lam_col = sel<D>(lam, rank);
    double gre, gim;
    cov_from_eig(vre, vim, lam_col, c, gre, gim);
    Base::store_apack(L, k, c, gre, gim);
    const double lnc = log_norm_of(lam, ba.norm_eps);
    if (!isfinite(lnc)) st |= PBBSS_ST_NONFINITE;
    if (last) {
      // numpy.linalg.eigh order: ascending scatter eigenvalues, eigenvectors in columns
      if (valid) {
        if (ba.out_eigvec) {
          double* ov = ba.out_eigvec + ((((size_t)b * K + k) * D + c.i) * D + rank) * 2;
          ov[0] = vre;
          ov[1] = vim;
        }
        if (ba.out_eigval && c.i == 0) ba.out_eigval[((size_t)b * K + k) * D + rank] = lam_col;
      }
      if (lane == 0 && ba.out_lognorm) ba.out_lognorm[(size_t)b * K + k] = lnc;
    }
    if (lane == 0) {
      L.rdet[k] = lnc;
      L.status[k] |= st;
      // mixture_model_utils.py:184-201 (the trainer always passes a saliency)
      L.wgt[k] = (a.weight_mode == PBBSS_WEIGHT_UNIFORM) ? 1.0 / K
                                                         : S / ((tot == 0.0) ? 1e-10 : tot);
    }
  }

  // model (V, lam) given by the caller -> B_k, ln c, weight (cbmm.py:21-58)
  static __device__ void prep_from_model(const BinghamArgs& ba, const Lds& L, int64_t b, int k,
                                         int lane) {
    const EmArgs& a = ba.em;
    const LaneIJ c = lane_ij(lane);
    const bool valid = c.i < D && c.j < D;
    double vre = 0.0, vim = 0.0, lam_col = 0.0;
    if (valid) {
      const double* v = ba.in_eigvec + ((((size_t)b * K + k) * D + c.i) * D + c.j) * 2;
      vre = v[0];
      vim = v[1];
    }
    if (c.j < D) lam_col = ba.in_eigval[((size_t)b * K + k) * D + c.j];
    double gre, gim;
    cov_from_eig(vre, vim, lam_col, c, gre, gim);
    Base::store_apack(L, k, c, gre, gim);
    int rank;
    double srt[D];
    sort_columns(lam_col, c, rank, srt);
    const double lnc = log_norm_of(srt, ba.norm_eps);
    if (lane == 0) {
      L.rdet[k] = lnc;
      if (ba.out_lognorm && a.iterations == 0) ba.out_lognorm[(size_t)b * K + k] = lnc;
      L.wgt[k] = a.in_weight ? a.in_weight[b * a.wb + k * a.wk] : 1.0 / K;
      if (!isfinite(lnc)) L.status[k] |= PBBSS_ST_NONFINITE;
    }
  }

  static __host__ __device__ size_t lds_bytes(int T) { return Base::lds_bytes(T); }

  static __device__ void run(const BinghamArgs& ba, char* smem) {
    const EmArgs& a = ba.em;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const Lds L = Base::carve(
        smem, a.T, SPILL ? a.scratch + (size_t)blockIdx.x * a.scratch_stride : nullptr);
    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
      __syncthreads();
      if (tid < K) L.status[tid] = 0;
      if (tid == 0) *L.flags = 0;
      __syncthreads();
      Base::phase_load(a, L, b, tid);
      __syncthreads();
      const bool model_in = (a.gamma0 == nullptr);
      if (model_in) {
        for (int k = wave; k < K; k += kEmWaves) prep_from_model(ba, L, b, k, lane);
      } else {
        phase_init_gamma(a, L, b, tid, wave, lane);
      }
      __syncthreads();
      for (int it = 0; it < a.iterations; ++it) {
        if (it > 0 || model_in) {
          phase_e<false>(ba, L, b, tid, wave, lane);
          __syncthreads();
        }
        switch (wave) {
          case 0: Base::template phase_m<0>(a, L, lane); break;
          case 1: Base::template phase_m<1>(a, L, lane); break;
          case 2: Base::template phase_m<2>(a, L, lane); break;
          default: Base::template phase_m<3>(a, L, lane); break;
        }
        __syncthreads();
        static_assert(K <= kEmWaves, "one class per wave");
        if (wave < K) factor_class(ba, L, b, wave, lane, it == a.iterations - 1);
        __syncthreads();
      }
      if (tid < K) {
        if (a.out_weight && a.iterations > 0) a.out_weight[(size_t)b * K + tid] = L.wgt[tid];
        if (a.out_status) a.out_status[(size_t)b * K + tid] = L.status[tid];
      }
      if (a.final_predict) phase_e<true>(ba, L, b, tid, wave, lane);
    }
  }
};

template <int D, int K, typename YS, bool SPILL>
__global__ void __launch_bounds__(kEmThreads, 1) cbmm_em_kernel(BinghamArgs ba) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  BinghamKernel<D, K, YS, SPILL>::run(ba, smem);
}

// find_eigenvalues_v3 on its own: one wave per spectrum, s (N, D) in any order -> lam (N, D) in
// the same order (complex_bingham.py:357-396 with the inverse permutation)
template <int D>
__global__ void __launch_bounds__(kWave) cbingham_find_eigenvalues_kernel(
    const double* s_in, int64_t N, double eps, double maxc, double* lam_out,
    int32_t* status_out) {
  const int lane = threadIdx.x;
  const LaneIJ c = lane_ij(lane);
  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    const double v = s_in[(size_t)n * D + (c.j < D ? c.j : 0)];
    int rank;
    double srt[D];
    BinghamKernel<D, 1, double, false>::sort_columns(v, c, rank, srt);
    double lam[D];
    const int st = bingham_find_eigenvalues<D>(srt, eps, maxc, lane, lam);
    if (c.i == 0 && c.j < D) lam_out[(size_t)n * D + c.j] = sel<D>(lam, rank);
    if (lane == 0) status_out[n] = st;
  }
}

}  // namespace pbbss
