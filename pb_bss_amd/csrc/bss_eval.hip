// BSS-Eval SDR / SIR / SAR on the device (include/pbbss.h, section V5-V9).
//
// Reference: pb_bss/evaluation/module_mir_eval.py:5-141, which hands the work to
// mir_eval.separation (bss_eval_sources and, for K + 1 estimates, _bss_decomp_mtifilt /
// _bss_source_crit): Vincent et al. 2006, BSS Eval 3.0.  The estimate e, zero-padded to
// N + L - 1 samples, is projected onto the L delays of reference j (P_j e) and onto the K L delays
// of all references (P_all e); the three ratios are
//   SDR = |P_j e|^2 / |e - P_j e|^2,  SIR = |P_j e|^2 / |P_all e - P_j e|^2,
//   SAR = |P_all e|^2 / |e - P_all e|^2.
//
// The phases, every one a launch set of its own (no workgroup ever waits for another one):
//   correlate   r_ij[l] = sum_n s_i[n] s_j[n + l], d_ie[l] = sum_n s_i[n] e[n + l], 0 <= l < L, and
//               |e|^2: a workgroup owns kBssCorrSpan samples of the first factor and stages them
//               with an L - 1 halo of the second in LDS; one lane per lag, direct summation;
//               span partials, added in span order by a finishing kernel.
//   assemble    the block-Toeplitz Gram matrix G (K L square) and the K Toeplitz diagonal blocks
//               (the single-source problems), padded with an identity to a multiple of the panel
//               width, and the right-hand sides.
//   factorise   blocked right-looking Cholesky G = R R^T, three launches per panel of 32 columns:
//               the diagonal block in the registers of one wave, the panel below it by forward
//               substitution (one row per lane), the trailing update on v_mfma_f64_16x16x4_f64
//               tiles (layout as in gauss_full.hip).  A pivot not larger than n 2^-52 times its
//               original diagonal entry marks the matrix as refused; nothing is divided by it and
//               every later kernel leaves that matrix alone.
//   solve       forward and backward substitution for kBssSolveRhs right-hand sides per workgroup.
//   synthesise  one pass over 0 .. N + L - 2 applies the filters (K L taps for P_all, L for P_j),
//               forms the residuals explicitly and reduces the five energies to span partials.
//   epilogue    one wave per item: dB tables, the mean-SIR search in itertools.permutations order
//               (first maximum, as np.argmax), status.
// float32 input is widened when it is staged; arithmetic is float64.  Every sum has a fixed
// order: results are bit-identical from call to call.
#include "bss_eval.hpp"

#include <math.h>

#include "carver.hpp"
#include "eval_dev.hpp"

namespace pbbss {
namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

static_assert(kBssMaxFilter == 2 * kBssThreads, "a correlation lane owns at most two lags");
static_assert(kBssSynSpan == 4 * kBssThreads, "a synthesis lane owns four output samples");
constexpr int kP = kBssPanel;
constexpr int kSynValues = 2;  // per estimate: |e - P_all|^2, |P_all|^2; then 3 per reference

struct BssDims {
  int64_t Bg, Br, chunksC, chunksS;
  int K, Ke, L, npa, np1, Jrr, Jre;
  size_t mat_stride;  // doubles of the K + 1 matrices of one reference item
  int A;              // synthesis partials per estimate and span
};

BssDims dims_of(const BssProblem& p, int64_t items) {
  BssDims d{};
  d.Bg = items;
  d.Br = p.ref_batch == 0 ? 1 : items;
  d.chunksC = bss_corr_chunks(p.N);
  d.chunksS = bss_syn_chunks(p.N, p.L);
  d.K = p.K, d.Ke = p.Ke, d.L = p.L;
  d.npa = bss_pad(p.K * p.L);
  d.np1 = bss_pad(p.L);
  d.Jrr = p.K * p.K;
  d.Jre = p.K * p.Ke + p.Ke;
  d.mat_stride = (size_t)d.npa * d.npa + (size_t)p.K * d.np1 * d.np1;
  d.A = kSynValues + 3 * p.K;
  return d;
}

void carve_work(Carver& c, const BssDims& d, BssWork& w) {
  w.p_rr = c.take<double>((size_t)d.Br * d.Jrr * d.chunksC * d.L);
  w.rr = c.take<double>((size_t)d.Br * d.Jrr * d.L);
  w.p_re = c.take<double>((size_t)d.Bg * d.Jre * d.chunksC * d.L);
  w.re = c.take<double>((size_t)d.Bg * d.Jre * d.L);
  w.mats = c.take<double>((size_t)d.Br * d.mat_stride);
  w.c_all = c.take<double>((size_t)d.Bg * d.Ke * d.npa);
  w.c_single = c.take<double>((size_t)d.Bg * d.Ke * d.K * d.np1);
  w.p_syn = c.take<double>((size_t)d.Bg * d.Ke * d.chunksS * d.A);
  w.fail = c.take<int32_t>((size_t)d.Br * (d.K + 1));
}

// ---- correlate ----------------------------------------------------------------------------
// grid (chunks, jobs, items).  mode 0: job i K + j is (s_i, s_j).  mode 1: job i Ke + e is
// (s_i, e_e), job K Ke + e is (e_e, e_e) with lag 0 only.  partials (items, jobs, chunks, L).
template <typename T>
__global__ __launch_bounds__(kBssThreads) void bss_corr_kernel(BssProblem g, int mode,
                                                               double* __restrict__ partials) {
  __shared__ double A[kBssCorrSpan];
  __shared__ double Bs[kBssCorrSpan + kBssMaxFilter];
  const int64_t w = blockIdx.x, b = blockIdx.z;
  const int job = blockIdx.y, tid = threadIdx.x;
  const int K = g.K, Ke = g.Ke, L = g.L;
  const T* ref = static_cast<const T*>(g.ref) + b * g.ref_batch;
  const T* est = static_cast<const T*>(g.est) + b * g.est_batch;
  const T *pa, *pb;
  int lags = L;
  if (mode == 0) {
    pa = ref + (job / K) * g.ref_row;
    pb = ref + (job % K) * g.ref_row;
  } else if (job < K * Ke) {
    pa = ref + (job / Ke) * g.ref_row;
    pb = est + (job % Ke) * g.est_row;
  } else {
    pa = pb = est + (job - K * Ke) * g.est_row;
    lags = 1;
  }
  const int64_t s0 = w * kBssCorrSpan;
  for (int t = tid; t < kBssCorrSpan; t += kBssThreads) {
    const int64_t n = s0 + t;
    A[t] = n < g.N ? (double)pa[n] : 0.0;
  }
  for (int t = tid; t < kBssCorrSpan + L - 1; t += kBssThreads) {
    const int64_t n = s0 + t;
    Bs[t] = n < g.N ? (double)pb[n] : 0.0;
  }
  __syncthreads();
  const int l0 = tid, l1 = tid + kBssThreads;
  const bool h0 = l0 < lags, h1 = l1 < lags;
  const double* b0 = Bs + (h0 ? l0 : 0);
  const double* b1 = Bs + (h1 ? l1 : 0);
  double acc0[4] = {0.0, 0.0, 0.0, 0.0}, acc1[4] = {0.0, 0.0, 0.0, 0.0};
  if (lags > kBssThreads) {
    for (int n = 0; n < kBssCorrSpan; n += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double a = A[n + u];
        acc0[u] = fma(a, b0[n + u], acc0[u]);
        acc1[u] = fma(a, b1[n + u], acc1[u]);
      }
    }
  } else {
    for (int n = 0; n < kBssCorrSpan; n += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc0[u] = fma(A[n + u], b0[n + u], acc0[u]);
    }
  }
  double* out = partials + (((int64_t)b * gridDim.y + job) * gridDim.x + w) * L;
  if (l0 < L) out[l0] = h0 ? (acc0[0] + acc0[1]) + (acc0[2] + acc0[3]) : 0.0;
  if (l1 < L) out[l1] = h1 ? (acc1[0] + acc1[1]) + (acc1[2] + acc1[3]) : 0.0;
}

// out[bj, l] = sum over the spans of partials[bj, chunk, l], in span order
__global__ __launch_bounds__(256) void bss_corr_finish_kernel(const double* __restrict__ partials,
                                                              int64_t total, int64_t chunks, int L,
                                                              double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int64_t bj = idx / L;
  const int l = (int)(idx - bj * L);
  out[idx] = span_sum(partials + bj * chunks * L + l, chunks, L);
}

// ---- assemble -----------------------------------------------------------------------------
// The matrices of reference item br: q = 0 the Gram matrix of all references (n = K L, padded to
// npa), q = 1 .. K the Toeplitz matrix of reference q - 1 (n = L, padded to np1), row-major.
struct BssMats {
  double* base;
  size_t stride;
  const double* rr;  // (Br, K K, L)
  int32_t* fail;     // (Br, K + 1) or null
  int K, L, npa, np1;
};

__device__ inline double* mat_of(const BssMats& m, int q, int64_t br, int& np, int& n) {
  np = q == 0 ? m.npa : m.np1;
  n = q == 0 ? m.K * m.L : m.L;
  return m.base + br * m.stride +
         (q == 0 ? (size_t)0 : (size_t)m.npa * m.npa + (size_t)(q - 1) * m.np1 * m.np1);
}

// r_ij[l - m] of reference item br
__device__ inline double gram_entry(const BssMats& m, int64_t br, int i, int l, int j, int mm) {
  const int d = l - mm;
  const int job = d >= 0 ? i * m.K + j : j * m.K + i;
  return m.rr[(br * m.K * m.K + job) * m.L + (d >= 0 ? d : -d)];
}

// grid (ceil(npa^2 / 256), matrices, Br)
__global__ __launch_bounds__(256) void bss_assemble_kernel(BssMats m) {
  const int q = blockIdx.y;
  const int64_t br = blockIdx.z;
  int np, n;
  double* M = mat_of(m, q, br, np, n);
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)np * np) return;
  const int r = (int)(idx / np), c = (int)(idx - (int64_t)r * np);
  double v;
  if (r >= n || c >= n)
    v = r == c ? 1.0 : 0.0;
  else if (q == 0)
    v = gram_entry(m, br, r / m.L, r % m.L, c / m.L, c % m.L);
  else
    v = gram_entry(m, br, q - 1, r, q - 1, c);
  M[idx] = v;
}

// right-hand sides from re (Bg, K Ke + Ke, L).  grid (ceil(K np1 / 256), Ke, Bg).
// c_all (Bg, Ke, npa), c_single (Bg, Ke, K, np1) or null.
__global__ __launch_bounds__(256) void bss_rhs_kernel(const double* __restrict__ re, int K, int Ke,
                                                      int L, int npa, int np1,
                                                      double* __restrict__ c_all,
                                                      double* __restrict__ c_single) {
  const int e = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int r = blockIdx.x * 256 + threadIdx.x;
  const double* reb = re + b * (K * Ke + Ke) * L;
  if (r < npa)
    c_all[(b * Ke + e) * npa + r] = r < K * L ? reb[((r / L) * Ke + e) * L + r % L] : 0.0;
  if (c_single && r < K * np1) {
    const int j = r / np1, l = r - j * np1;
    c_single[((b * Ke + e) * K + j) * np1 + l] = l < L ? reb[(j * Ke + e) * L + l] : 0.0;
  }
}

// ---- factorise ----------------------------------------------------------------------------
// diagonal block of panel k.  grid (1, K + 1, Br), one wave; lane r (and its mirror r + 32) holds
// row r of the block.
__global__ __launch_bounds__(64) void bss_chol_diag_kernel(BssMats m, int k) {
  const int q = blockIdx.y;
  const int64_t br = blockIdx.z;
  int np, n;
  double* M = mat_of(m, q, br, np, n);
  int32_t* fail = m.fail + br * (m.K + 1) + q;
  if (k * kP >= np || *fail) return;
  const int lane = threadIdx.x, r = lane & (kP - 1);
  const int row = k * kP + r;
  double a[kP];
  double* Mr = M + (size_t)row * np + k * kP;
#pragma unroll
  for (int c = 0; c < kP; ++c) a[c] = Mr[c];
  // the pivot's original diagonal entry: r_ii[0] (1 in the padding)
  double od = 1.0;
  if (row < n) {
    const int i = q == 0 ? row / m.L : q - 1;
    od = m.rr[(br * m.K * m.K + i * m.K + i) * m.L];
  }
  const double thr = (double)n * 0x1p-52 * od;
  bool refused = false;
#pragma unroll
  for (int j = 0; j < kP; ++j) {
    if (!refused) {
      const double pj = __shfl(a[j], j, 64), tj = __shfl(thr, j, 64);
      if (!(pj > tj)) {  // also a NaN
        refused = true;
      } else {
        const double d = sqrt(pj);
        a[j] = r == j ? d : a[j] / d;
#pragma unroll
        for (int c = j + 1; c < kP; ++c) a[c] = fma(-a[j], __shfl(a[j], c, 64), a[c]);
      }
    }
  }
  if (refused) {
    if (lane == 0) *fail = 1;
    return;
  }
  if (lane < kP) {
#pragma unroll
    for (int c = 0; c < kP; ++c)
      if (c <= r) Mr[c] = a[c];
  }
}

// rows below the diagonal block: X L11^T = A21, one row per lane.  grid (row tiles of 64, K + 1, Br)
__global__ __launch_bounds__(64) void bss_chol_trsm_kernel(BssMats m, int k) {
  __shared__ double L11[kP][kP + 1];
  const int q = blockIdx.y;
  const int64_t br = blockIdx.z;
  int np, n;
  double* M = mat_of(m, q, br, np, n);
  const int row = (k + 1) * kP + blockIdx.x * 64 + threadIdx.x;
  if ((k + 1) * kP + (int)blockIdx.x * 64 >= np || m.fail[br * (m.K + 1) + q]) return;
  for (int t = threadIdx.x; t < kP * kP; t += 64)
    L11[t / kP][t % kP] = M[(size_t)(k * kP + t / kP) * np + k * kP + t % kP];
  __syncthreads();
  if (row >= np) return;
  double* Mr = M + (size_t)row * np + k * kP;
  double x[kP];
#pragma unroll
  for (int c = 0; c < kP; ++c) x[c] = Mr[c];
#pragma unroll
  for (int j = 0; j < kP; ++j) {
    double s = x[j];
#pragma unroll
    for (int c = 0; c < j; ++c) s = fma(-x[c], L11[j][c], s);
    x[j] = s / L11[j][j];
  }
#pragma unroll
  for (int c = 0; c < kP; ++c) Mr[c] = x[c];
}

// trailing update A22 -= L21 L21^T on the lower triangle, a 32 x 32 tile per workgroup, a
// 16 x 16 MFMA tile per wave.  grid (T (T + 1) / 2 tiles of the largest matrix, K + 1, Br)
__global__ __launch_bounds__(256) void bss_chol_update_kernel(BssMats m, int k) {
  const int q = blockIdx.y;
  const int64_t br = blockIdx.z;
  int np, n;
  double* M = mat_of(m, q, br, np, n);
  const int t0 = (k + 1) * kP;
  const int T = (np - t0) / kP;
  const int bx = blockIdx.x;
  if (T <= 0 || bx >= T * (T + 1) / 2 || m.fail[br * (m.K + 1) + q]) return;
  int ti = (int)((sqrt(8.0 * bx + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > bx) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= bx) ++ti;
  const int tj = bx - ti * (ti + 1) / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = wave >> 1, wj = wave & 1;
  if (ti == tj && wj > wi) return;  // strictly above the diagonal
  const int rowA = t0 + kP * ti + 16 * wi, rowB = t0 + kP * tj + 16 * wj;
  const double* pa = M + (size_t)(rowA + (lane & 15)) * np + k * kP + (lane >> 4);
  const double* pb = M + (size_t)(rowB + (lane & 15)) * np + k * kP + (lane >> 4);
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < kP / 4; ++s)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * s], pb[4 * s], acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    M[(size_t)(rowA + 4 * r + (lane >> 4)) * np + rowB + (lane & 15)] -= acc[r];
}

// ---- solve --------------------------------------------------------------------------------
// R R^T c = d in place for the right-hand sides of matrix (q, br): q = 0 the rows of c_all,
// q >= 1 row q - 1 of c_single, of the `nvec` (item, estimate) pairs from `first` on.
// grid (ceil(nvec / kBssSolveRhs), K + 1, Br); wave v runs the diagonal block of vector v.
__global__ __launch_bounds__(kBssThreads) void bss_solve_kernel(BssMats m, int shared, int nvec,
                                                                int Ke, double* __restrict__ c_all,
                                                                double* __restrict__ c_single) {
  __shared__ double xk[kBssSolveRhs][kP];
  const int q = blockIdx.y;
  const int64_t br = blockIdx.z;
  int np, n;
  const double* M = mat_of(m, q, br, np, n);
  const int v0 = blockIdx.x * kBssSolveRhs;
  const int nact = nvec - v0 < kBssSolveRhs ? nvec - v0 : kBssSolveRhs;
  if (nact <= 0 || m.fail[br * (m.K + 1) + q]) return;
  const int64_t first = shared ? 0 : br * Ke;
  double* x[kBssSolveRhs];
#pragma unroll
  for (int v = 0; v < kBssSolveRhs; ++v) {
    const int64_t vec = first + v0 + (v < nact ? v : 0);
    x[v] = q == 0 ? c_all + vec * m.npa : c_single + (vec * m.K + (q - 1)) * m.np1;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & (kP - 1);
  if (tid < kBssSolveRhs * kP) xk[tid / kP][tid % kP] = 0.0;
  const int P = np / kP;
  double* xw = x[0];
#pragma unroll
  for (int v = 1; v < kBssSolveRhs; ++v)
    if (wave == v) xw = x[v];

  for (int k = 0; k < P; ++k) {  // R y = d
    const int k0 = k * kP;
    __syncthreads();
    if (wave < nact) {
      const double* Mr = M + (size_t)(k0 + r) * np + k0;
      double a[kP];
#pragma unroll
      for (int c = 0; c < kP; ++c) a[c] = Mr[c];
      const double rdg = 1.0 / Mr[r];
      double b = xw[k0 + r];
#pragma unroll
      for (int j = 0; j < kP; ++j) {
        const double xj = __shfl(b * rdg, j, 64);
        if (r > j) b = fma(-a[j], xj, b);
      }
      b *= rdg;
      if (lane < kP) {
        xk[wave][r] = b;
        xw[k0 + r] = b;
      }
    }
    __syncthreads();
    for (int row = k0 + kP + tid; row < np; row += kBssThreads) {
      const double* Lr = M + (size_t)row * np + k0;
      double s[kBssSolveRhs];
#pragma unroll
      for (int v = 0; v < kBssSolveRhs; ++v) s[v] = x[v][row];
#pragma unroll
      for (int c = 0; c < kP; ++c) {
        const double l = Lr[c];
#pragma unroll
        for (int v = 0; v < kBssSolveRhs; ++v) s[v] = fma(-l, xk[v][c], s[v]);
      }
#pragma unroll
      for (int v = 0; v < kBssSolveRhs; ++v)
        if (v < nact) x[v][row] = s[v];
    }
  }
  for (int k = P - 1; k >= 0; --k) {  // R^T c = y
    const int k0 = k * kP;
    __syncthreads();
    if (wave < nact) {
      double a[kP];  // column r of the diagonal block
#pragma unroll
      for (int j = 0; j < kP; ++j) a[j] = M[(size_t)(k0 + j) * np + k0 + r];
      const double rdg = 1.0 / M[(size_t)(k0 + r) * np + k0 + r];
      double b = xw[k0 + r];
#pragma unroll
      for (int j = kP - 1; j >= 0; --j) {
        const double xj = __shfl(b * rdg, j, 64);
        if (r < j) b = fma(-a[j], xj, b);
      }
      b *= rdg;
      if (lane < kP) {
        xk[wave][r] = b;
        xw[k0 + r] = b;
      }
    }
    __syncthreads();
    for (int row = tid; row < k0; row += kBssThreads) {
      double s[kBssSolveRhs];
#pragma unroll
      for (int v = 0; v < kBssSolveRhs; ++v) s[v] = x[v][row];
#pragma unroll
      for (int c = 0; c < kP; ++c) {
        const double l = M[(size_t)(k0 + c) * np + row];
#pragma unroll
        for (int v = 0; v < kBssSolveRhs; ++v) s[v] = fma(-l, xk[v][c], s[v]);
      }
#pragma unroll
      for (int v = 0; v < kBssSolveRhs; ++v)
        if (v < nact) x[v][row] = s[v];
    }
  }
}

// ---- synthesise ---------------------------------------------------------------------------
// grid (chunksS, Ke, Bg).  c_all (.., Ke, ld_all): K blocks of L taps; c_single (.., Ke, K,
// ld_single).  partials (Bg, Ke, chunksS, 2 + 3 K): |e - P_all|^2, |P_all|^2, then per reference
// j |P_j|^2, |P_all - P_j|^2, |e - P_j|^2 (zero for the pairs a call without the search skips).
template <typename T>
__global__ __launch_bounds__(kBssThreads) void bss_synth_kernel(BssProblem g,
                                                                const double* __restrict__ c_all,
                                                                int64_t ld_all,
                                                                const double* __restrict__ c_single,
                                                                int64_t ld_single,
                                                                double* __restrict__ partials) {
  __shared__ double S[kBssSynSpan + kBssMaxFilter];
  __shared__ double C[kBssMaxFilter];
  __shared__ double red[kBssThreads / 64][3];
  const int64_t w = blockIdx.x, b = blockIdx.z;
  const int e = blockIdx.y, tid = threadIdx.x;
  const int K = g.K, Ke = g.Ke, L = g.L;
  const T* ref = static_cast<const T*>(g.ref) + b * g.ref_batch;
  const T* est = static_cast<const T*>(g.est) + b * g.est_batch + e * g.est_row;
  const double* ca = c_all + (b * Ke + e) * ld_all;
  const double* cs = c_single + (b * Ke + e) * K * ld_single;
  const int64_t n0 = w * kBssSynSpan;
  const int A = kSynValues + 3 * K;
  double* out = partials + ((b * Ke + e) * gridDim.x + w) * A;

  // S[t] = s[n0 - (L - 1) + t], so output sample n0 + u reads S[u + L - 1 - l] for tap l
  auto filter = [&](const T* s, const double* taps, double (&p)[4]) {
    __syncthreads();
    for (int t = tid; t < kBssSynSpan + L - 1; t += kBssThreads) {
      const int64_t n = n0 - (L - 1) + t;
      S[t] = n >= 0 && n < g.N ? (double)s[n] : 0.0;
    }
    for (int l = tid; l < L; l += kBssThreads) C[l] = taps[l];
    __syncthreads();
    const double* Su = S + tid + L - 1;
    for (int l = 0; l < L; ++l) {
      const double c = C[l];
#pragma unroll
      for (int mm = 0; mm < 4; ++mm) p[mm] = fma(c, Su[mm * kBssThreads - l], p[mm]);
    }
  };
  // workgroup sums of up to three values, the waves added in order; valid on lane 0
  auto block_sum = [&](double (&v)[3]) {
    const int lane = tid & 63, wv = tid >> 6;
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double s = wave_sum(v[a]);
      if (lane == 0) red[wv][a] = s;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double s = red[0][a];
#pragma unroll
      for (int x = 1; x < kBssThreads / 64; ++x) s += red[x][a];
      v[a] = s;
    }
  };

  double pall[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < K; ++i) filter(ref + i * g.ref_row, ca + i * L, pall);
  double ev[4];
#pragma unroll
  for (int mm = 0; mm < 4; ++mm) {
    const int64_t n = n0 + tid + mm * kBssThreads;
    ev[mm] = n < g.N ? (double)est[n] : 0.0;
  }
  double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int mm = 0; mm < 4; ++mm) {
    const double d = ev[mm] - pall[mm];
    v[0] = fma(d, d, v[0]);
    v[1] = fma(pall[mm], pall[mm], v[1]);
  }
  block_sum(v);
  if (tid == 0) out[0] = v[0], out[1] = v[1];
  for (int j = 0; j < K; ++j) {
    if (!g.permute && j != e) {
      if (tid < 3) out[kSynValues + 3 * j + tid] = 0.0;
      continue;
    }
    double pj[4] = {0.0, 0.0, 0.0, 0.0};
    filter(ref + j * g.ref_row, cs + j * ld_single, pj);
    v[0] = v[1] = v[2] = 0.0;
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
      const double da = pall[mm] - pj[mm], de = ev[mm] - pj[mm];
      v[0] = fma(pj[mm], pj[mm], v[0]);
      v[1] = fma(da, da, v[1]);
      v[2] = fma(de, de, v[2]);
    }
    block_sum(v);
    if (tid == 0) {
      out[kSynValues + 3 * j] = v[0];
      out[kSynValues + 3 * j + 1] = v[1];
      out[kSynValues + 3 * j + 2] = v[2];
    }
  }
}

// ---- epilogue -----------------------------------------------------------------------------
__device__ inline double safe_db(double num, double den) {
  return den == 0.0 ? (double)INFINITY : 10.0 * log10(num / den);
}

// one wave per item.  rr / re / fail null: filters came from the caller, status 0.
__global__ __launch_bounds__(64) void bss_epilogue_kernel(
    const double* __restrict__ p_syn, int64_t chunksS, int K, int Ke, int L, int permute,
    const double* __restrict__ rr, const double* __restrict__ re, const int32_t* __restrict__ fail,
    int shared, BssOutputs o) {
  constexpr int MK = kBssMaxSources;
  __shared__ double tab[3][MK * MK];
  __shared__ int chosen[MK];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int A = kSynValues + 3 * K;
  for (int qd = lane; qd < Ke * K; qd += 64) {
    const int e = qd / K, j = qd - e * K;
    const double* pe = p_syn + (b * Ke + e) * chunksS * A;
    double sdr = NAN, sir = NAN, sar = NAN;
    if (permute || e == j) {
      const double ea = span_sum(pe, chunksS, A), aa = span_sum(pe + 1, chunksS, A);
      const double jj = span_sum(pe + kSynValues + 3 * j, chunksS, A);
      const double aj = span_sum(pe + kSynValues + 3 * j + 1, chunksS, A);
      const double ej = span_sum(pe + kSynValues + 3 * j + 2, chunksS, A);
      sdr = safe_db(jj, ej), sir = safe_db(jj, aj), sar = safe_db(aa, ea);
    }
    tab[0][qd] = sdr, tab[1][qd] = sir, tab[2][qd] = sar;
    if (o.tables) {
      double* t = o.tables + b * 3 * Ke * K;
      t[qd] = sdr, t[Ke * K + qd] = sir, t[2 * Ke * K + qd] = sar;
    }
  }
  __syncthreads();
  if (lane == 0) {
    unsigned st = 0;
    if (rr) {
      const int64_t br = shared ? 0 : b;
      for (int q = 0; q <= K; ++q)
        if (fail[br * (K + 1) + q]) st |= PBBSS_ST_NOT_POSDEF;
      for (int i = 0; i < K; ++i)
        if (rr[(br * K * K + i * K + i) * L] == 0.0) st |= PBBSS_ST_ZERO_SIGNAL;
      for (int e = 0; e < Ke; ++e)
        if (re[(b * (K * Ke + Ke) + K * Ke + e) * L] == 0.0) st |= PBBSS_ST_ZERO_SIGNAL;
    }
    o.status[b] = (int32_t)st;
  }

  if (permute) {
    // radix[k]: picks that share their first k + 1 entries
    int radix[kSxrMaxTargets];
#pragma unroll
    for (int k = kSxrMaxTargets - 1; k >= 0; --k) {
      radix[k] = 1;
      if (k < K - 1) radix[k] = radix[k + 1 < kSxrMaxTargets ? k + 1 : k] * (Ke - 1 - k);
    }
    const int P = radix[0] * Ke;
    double best = 0.0;
    int best_p = 0x7fffffff;
    for (int p = lane; p < P; p += 64) {
      int sel[kSxrMaxTargets];
      unrank_selection(p, K, Ke, radix, sel);
      double v[kSxrMaxTargets];
#pragma unroll
      for (int k = 0; k < kSxrMaxTargets; ++k) v[k] = k < K ? tab[1][sel[k] * K + k] : 0.0;
      double total;  // np.mean of K values
      if (K == 8) {
        total = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
      } else {
        total = 0.0;
#pragma unroll
        for (int k = 0; k < kSxrMaxTargets - 1; ++k)
          if (k < K) total += v[k];
      }
      total /= (double)K;
      if (best_p == 0x7fffffff || ahead(total, p, best, best_p)) {
        best = total;
        best_p = p;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_down(best, off, 64);
      const int op = __shfl_down(best_p, off, 64);
      if (op != 0x7fffffff && (best_p == 0x7fffffff || ahead(ov, op, best, best_p))) {
        best = ov;
        best_p = op;
      }
    }
    if (lane == 0) {
      int sel[kSxrMaxTargets];
      unrank_selection(best_p, K, Ke, radix, sel);
#pragma unroll
      for (int k = 0; k < kSxrMaxTargets; ++k)
        if (k < K) chosen[k] = sel[k];
    }
  } else if (lane < K) {
    chosen[lane] = lane;
  }
  __syncthreads();
  if (lane < K) {
    const int t = chosen[lane] * K + lane;
    o.sdr[b * K + lane] = tab[0][t];
    o.sir[b * K + lane] = tab[1][t];
    o.sar[b * K + lane] = tab[2][t];
    o.selection[b * K + lane] = chosen[lane];
  }
}

// ---- launchers ----------------------------------------------------------------------------
inline int hip_ok() { return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP; }
inline unsigned blocks_for(int64_t total) { return (unsigned)((total + 255) / 256); }

void launch_corr(const BssProblem& p, int mode, int jobs, int64_t items, int64_t chunks,
                 double* partials, double* out, hipStream_t s) {
  const dim3 grid((unsigned)chunks, (unsigned)jobs, (unsigned)items), block(kBssThreads);
  if (p.is_f64)
    hipLaunchKernelGGL((bss_corr_kernel<double>), grid, block, 0, s, p, mode, partials);
  else
    hipLaunchKernelGGL((bss_corr_kernel<float>), grid, block, 0, s, p, mode, partials);
  const int64_t total = items * jobs * p.L;
  hipLaunchKernelGGL(bss_corr_finish_kernel, dim3(blocks_for(total)), dim3(256), 0, s, partials,
                     total, chunks, p.L, out);
}

void launch_correlations(const BssProblem& p, const BssDims& d, const BssWork& w, hipStream_t s) {
  launch_corr(p, 0, d.Jrr, d.Br, d.chunksC, w.p_rr, w.rr, s);
  launch_corr(p, 1, d.Jre, d.Bg, d.chunksC, w.p_re, w.re, s);
}

// the problem of items [b0, b0 + items)
BssProblem sub_problem(const BssProblem& p, int64_t b0, int64_t items) {
  BssProblem g = p;
  const size_t size = p.is_f64 ? 8 : 4;
  g.ref = static_cast<const char*>(p.ref) + (size_t)(b0 * p.ref_batch) * size;
  g.est = static_cast<const char*>(p.est) + (size_t)(b0 * p.est_batch) * size;
  g.B = items;
  return g;
}

// the five events around the four phases of a timed call
struct PhaseEvents {
  hipEvent_t ev[5] = {};
  bool create() {
    for (hipEvent_t& e : ev)
      if (hipEventCreate(&e) != hipSuccess) return false;
    return true;
  }
  ~PhaseEvents() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// w: a workspace carved for at least p.B items.  phase_ms (or null): device time of correlate +
// assemble, factorise, solve, synthesise + epilogue is ADDED to its four entries; the call then
// waits for the group.
int run_group(const BssProblem& p, const BssFilters* filters, const BssWork& w,
              const BssOutputs& o, float* phase_ms, hipStream_t s) {
  PhaseEvents events;
  if (phase_ms && !events.create()) return PBBSS_ERR_HIP;
  hipEvent_t* ev = events.ev;
  auto mark = [&](int i) {
    if (phase_ms) (void)hipEventRecord(ev[i], s);
  };
  mark(0);
  const BssDims d = dims_of(p, p.B);
  const int shared = p.ref_batch == 0;
  const double *c_all, *c_single;
  int64_t ld_all, ld_single;
  if (!filters) {
    launch_correlations(p, d, w, s);
    if (hipMemsetAsync(w.fail, 0, (size_t)d.Br * (d.K + 1) * sizeof(int32_t), s) != hipSuccess)
      return PBBSS_ERR_HIP;
    const BssMats m{w.mats, d.mat_stride, w.rr, w.fail, d.K, d.L, d.npa, d.np1};
    const unsigned nq = (unsigned)d.K + 1, Br = (unsigned)d.Br;
    hipLaunchKernelGGL(bss_assemble_kernel, dim3(blocks_for((int64_t)d.npa * d.npa), nq, Br),
                       dim3(256), 0, s, m);
    hipLaunchKernelGGL(bss_rhs_kernel, dim3(blocks_for((int64_t)d.K * d.np1), d.Ke, (unsigned)d.Bg),
                       dim3(256), 0, s, w.re, d.K, d.Ke, d.L, d.npa, d.np1, w.c_all, w.c_single);
    mark(1);
    const int P = d.npa / kP;
    for (int k = 0; k < P; ++k) {
      hipLaunchKernelGGL(bss_chol_diag_kernel, dim3(1, nq, Br), dim3(64), 0, s, m, k);
      const int below = d.npa - (k + 1) * kP;
      if (below <= 0) break;
      hipLaunchKernelGGL(bss_chol_trsm_kernel, dim3((below + 63) / 64, nq, Br), dim3(64), 0, s, m,
                         k);
      const int T = below / kP;
      hipLaunchKernelGGL(bss_chol_update_kernel, dim3(T * (T + 1) / 2, nq, Br), dim3(256), 0, s, m,
                         k);
    }
    mark(2);
    const int nvec = shared ? (int)(d.Bg * d.Ke) : d.Ke;
    hipLaunchKernelGGL(bss_solve_kernel, dim3((nvec + kBssSolveRhs - 1) / kBssSolveRhs, nq, Br),
                       dim3(kBssThreads), 0, s, m, shared, nvec, d.Ke, w.c_all, w.c_single);
    mark(3);
    c_all = w.c_all, c_single = w.c_single;
    ld_all = d.npa, ld_single = d.np1;
  } else {
    mark(1), mark(2), mark(3);
    c_all = filters->all, c_single = filters->single;
    ld_all = (int64_t)d.K * d.L, ld_single = d.L;
  }
  const dim3 sgrid((unsigned)d.chunksS, (unsigned)d.Ke, (unsigned)d.Bg);
  if (p.is_f64)
    hipLaunchKernelGGL((bss_synth_kernel<double>), sgrid, dim3(kBssThreads), 0, s, p, c_all,
                       ld_all, c_single, ld_single, w.p_syn);
  else
    hipLaunchKernelGGL((bss_synth_kernel<float>), sgrid, dim3(kBssThreads), 0, s, p, c_all, ld_all,
                       c_single, ld_single, w.p_syn);
  hipLaunchKernelGGL(bss_epilogue_kernel, dim3((unsigned)d.Bg), dim3(64), 0, s, w.p_syn, d.chunksS,
                     d.K, d.Ke, d.L, p.permute, filters ? nullptr : w.rr,
                     filters ? nullptr : w.re, filters ? nullptr : w.fail, shared, o);
  mark(4);
  if (phase_ms) {
    (void)hipEventSynchronize(ev[4]);
    for (int i = 0; i < 4; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) phase_ms[i] += ms;
    }
  }
  return hip_ok();
}

}  // namespace

void bss_carve(Carver& c, const BssProblem& p, int64_t items, BssWork& w) {
  carve_work(c, dims_of(p, items), w);
}

size_t bss_group_work(const BssProblem& p, int64_t items) {
  BssWork w{};
  Carver measure;
  bss_carve(measure, p, items, w);
  return measure.off;
}

int64_t bss_group_items(const BssProblem& p) {
  int64_t items = p.B < kBssMaxGroup ? p.B : kBssMaxGroup;
  while (items > 1 && bss_group_work(p, items) > kBssGroupBytes) items = (items + 1) / 2;
  return items;
}

int launch_bss_eval(const BssProblem& p, const BssFilters* filters, const BssWork& work,
                    int64_t group, const BssOutputs& out, float* phase_ms, hipStream_t s) {
  for (int64_t b0 = 0; b0 < p.B; b0 += group) {
    const int64_t items = p.B - b0 < group ? p.B - b0 : group;
    const BssProblem g = sub_problem(p, b0, items);
    BssFilters f{};
    if (filters) {
      f.all = filters->all + b0 * p.Ke * p.K * p.L;
      f.single = filters->single + b0 * p.Ke * p.K * p.L;
    }
    BssOutputs o = out;
    o.sdr += b0 * p.K, o.sir += b0 * p.K, o.sar += b0 * p.K, o.selection += b0 * p.K;
    if (o.tables) o.tables += b0 * 3 * p.Ke * p.K;
    o.status += b0;
    const int rc = run_group(g, filters ? &f : nullptr, work, o, phase_ms, s);
    if (rc != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}

int launch_bss_system(const BssProblem& p, const BssWork& w, int64_t group, double* out_G,
                      double* out_D, hipStream_t s) {
  const int n = p.K * p.L;
  const int shared = p.ref_batch == 0;
  for (int64_t b0 = 0; b0 < p.B; b0 += group) {
    const int64_t items = p.B - b0 < group ? p.B - b0 : group;
    const BssProblem g = sub_problem(p, b0, items);
    const BssDims d = dims_of(g, items);
    launch_correlations(g, d, w, s);
    // unpadded: the matrix and the right-hand sides as NumPy wants them
    if (!shared || b0 == 0) {
      const BssMats m{out_G + (shared ? 0 : b0) * (size_t)n * n, (size_t)n * n, w.rr, nullptr, d.K,
                      d.L, n, d.L};
      hipLaunchKernelGGL(bss_assemble_kernel, dim3(blocks_for((int64_t)n * n), 1, (unsigned)d.Br),
                         dim3(256), 0, s, m);
    }
    hipLaunchKernelGGL(bss_rhs_kernel, dim3(blocks_for(n), d.Ke, (unsigned)d.Bg), dim3(256), 0, s,
                       w.re, d.K, d.Ke, d.L, n, d.L, out_D + b0 * p.Ke * n, (double*)nullptr);
    if (hip_ok() != PBBSS_OK) return PBBSS_ERR_HIP;
  }
  return PBBSS_OK;
}

}  // namespace pbbss
