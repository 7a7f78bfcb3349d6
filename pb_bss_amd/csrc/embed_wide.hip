// Real-embedding mixtures with 9 <= K <= 64 classes on the FP64 matrix pipe of gfx950.
//
// Reference: distribution/vmfmm.py:42-148, gmm.py:33-171 (the EM loops), von_mises_fisher.py:62-78,
// :119-144, gaussian.py:76-97, :108-137, :152-193 (class log-pdfs and weighted fits),
// mixture_model_utils.py:7-55 (log_pdf_to_affiliation: subtract the class maximum, exponentiate,
// multiply by the weight, divide by max(sum, tiny)).
//
// embed.hip keeps one accumulator per class in every lane, which stops at eight classes.  Here both
// contractions of an EM iteration are v_mfma_f64_16x16x4_f64 tiles (lane l feeds A[i = l % 16]
// [k = l / 16] and B[k = l / 16][j = l % 16] and holds D[4 r + l / 16][l % 16] in accumulator
// register r, see gauss_full.hip):
//   E  D[sample][class] = sum_e y'[sample][e] m[class][e], features in steps of four.  A row's
//      classes lie across the 16 lanes of a DPP row and the KT = ceil(K / 16) class tiles; the
//      maximum and the sum of the softmax are DPP row reductions.
//   M  D[class][column] = sum_n w[class][n] Y[n][column], samples in steps of four, over the LDS
//      columns [y' (E, padded to four) ; 1 ; |y'|^2].  Register r of the E-step tile IS the A
//      operand of the sample group 4 r .. 4 r + 3 (A[class = l % 16][sample = l / 16]): the
//      posteriors never change lanes between the two contractions.
// A workgroup (four wavefronts) walks a chunk of rows in blocks of R = 64 / 32 / 16: the block is
// read once from the caller's row-major array (float32 or float64, coalesced), widened and
// shifted into an LDS tile, and every wavefront runs both contractions on its own 16 rows.  No
// transposed copy, no (B, K, N) affiliation array between the two steps.
//   y' = y - g with g the column mean of the mixture's rows, taken once per fit (Gaussians:
//   |y - m|^2 is expanded as |y'|^2 - 2 y'.m' + |m'|^2, and the second moment is taken about g
//   and corrected in the finalize.  The shifted tile is shared by all classes, so g cannot follow
//   the classes: a class loses (|mean_k - g| / spread_k)^2 eps, which is small for clusters a few
//   spreads apart and inherent for clusters far apart.  A weightless outlier moves g by its
//   distance / N only, where any single row taken as g could BE the outlier);
//   vMF: y' = y, the dot products and the M-step weights carry 1 / |y_n| (vmfmm.py:76-78) and the
//   "1" column holds |y_n| so that the weight sums come out unscaled.
// Accumulators: KT x ETW M-step tiles per wavefront with ETW <= 16 / KT (64 doubles per lane);
// a shape with more column tiles (K E large) splits them over gridDim.z, each slice repeating the
// E-step.  Class means sit in LDS where they fit beside the row tile, else they are read through
// the L2 from the padded copy the model kernel writes.  Chunk partials are summed in a fixed
// order by wide_finalize_kernel (one workgroup per class): bit-reproducible, no atomics.
#include "embed_wide.hpp"
#include <cmath>
#include "pbbss_dev.hpp"
#include "embed_dev.hpp"
#include "dispatch.hpp"

namespace pbbss {
namespace {

constexpr int kWT = 256;  // four wavefronts
constexpr double kLn2Pi = 1.8378770664093454;
constexpr double kNoClass = -1.0e300;  // log-pdf of the padding classes of the last tile
typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ size_t aff_index(int64_t b, int k, int64_t n, int K, int64_t N,
                                            int64_t Tin) {
  const int64_t f = n / Tin;
  return (size_t)b * K * N + (size_t)f * K * Tin + (size_t)k * Tin + (size_t)(n - f * Tin);
}

// all-reduce over the 16 lanes of a DPP row
template <typename Op>
__device__ __forceinline__ double row16_allreduce(double v, Op op) {
  v = op(v, dpp_f64<kDppQuadXor1, 0xF>(v, v));
  v = op(v, dpp_f64<kDppQuadXor2, 0xF>(v, v));
  v = op(v, dpp_f64<kDppRowHalfMirror, 0xF>(v, v));
  v = op(v, dpp_f64<kDppRowMirror, 0xF>(v, v));
  return v;
}
__device__ __forceinline__ double row16_sum(double v) {
  return row16_allreduce(v, [](double x, double y) { return x + y; });
}
__device__ __forceinline__ double row16_max(double v) {
  return row16_allreduce(v, [](double x, double y) { return fmax(x, y); });
}

struct SweepArgs {
  const void* y;       // (B, N, E) row-major
  int64_t N, L, Tin;   // rows per mixture, rows per chunk (multiple of R), output layout
  int E, E4, K, R, LDY, ET, C, EC, ybuf;
  const double* gamma;  // (B, K, N) through aff_index: weights of this sweep, or null: the model
  const double* sal;    // (B, N) or null
  const double* shift;  // (B, E4) or null
  int vmf, mnorm, square, mu_lds, accumulate;
  const double* mup;    // (B, NM KP, E4) padded class rows
  const double* cst;    // (B, 4, KP): a, b, c of lp = a (rs dot) + c q + b, and the class weight
  double out_scale;
  double* out_lp;
  double* out_aff;
  double* part;         // (B, C, K, EC)
};

// acc[m KT + c][r] += sum_e y'[row0 + 4 r + l / 16][e] mu[(m KT + c) 16 + l % 16][e]
template <int NT>
__device__ __forceinline__ void wide_dots(const double* yt, int LDY, int row0, const double* mu,
                                          int LDM, int E4, int lane, d4 (&acc)[NT]) {
  const double* ap = yt + (size_t)(row0 + (lane & 15)) * LDY + (lane >> 4);
  const double* bp = mu + (size_t)(lane & 15) * LDM + (lane >> 4);
  for (int s = 0; s < E4; s += 4) {
    const double av = ap[s];
#pragma unroll
    for (int c = 0; c < NT; ++c)
      acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bp[(size_t)c * 16 * LDM + s], acc[c], 0, 0, 0);
  }
}

// NM = 1: vMF / spherical Gaussian; NM = 2: DiagonalGaussian.log_pdf (E-step only)
// ETW: column tiles of the M-step a workgroup accumulates (KT ETW <= 16 tiles = 64 doubles a lane)
template <typename TS, int KT, int NM, int ETW>
__global__ void __launch_bounds__(kWT) wide_sweep_kernel(const SweepArgs a) {
  constexpr int KP = 16 * KT;
  constexpr bool DIAG = NM == 2;
  extern __shared__ double sm[];
  const int R = a.R, LDY = a.LDY, E = a.E, E4 = a.E4, K = a.K, LDM = a.E4 + 1;
  double* ytile = sm;               // [R][LDY]; at the end [KP][16 nt] for the wave reduction
  double* rowaux = sm + a.ybuf;     // [R][2]: M-step row weight, E-step row scale
  double* gsh = rowaux + 2 * R;     // [E4] common shift
  double* mul = gsh + E4;           // [NM KP][LDM] class rows (mu_lds)
  const int64_t b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int l16 = lane & 15, lg = lane >> 4;
  const int t0 = blockIdx.z * ETW;
  const int nt = (a.ET - t0 < ETW) ? a.ET - t0 : ETW;
  const int64_t n0 = (int64_t)blockIdx.x * a.L;
  const int64_t n1 = (n0 + a.L < a.N) ? n0 + a.L : a.N;
  const bool model = a.gamma == nullptr;
  const double* mug = a.mup + (size_t)b * NM * KP * E4;

  for (int i = tid; i < R * LDY; i += kWT) ytile[i] = 0.0;
  for (int i = tid; i < E4; i += kWT) gsh[i] = a.shift ? a.shift[(size_t)b * E4 + i] : 0.0;
  if (model && a.mu_lds) {
    for (int i = tid; i < NM * KP * E4; i += kWT) {
      const int r = i / E4, d = i - r * E4;
      mul[r * LDM + d] = mug[i];
    }
  }
  double ca[KT], cb[KT], cc[KT], cw[KT];
#pragma unroll
  for (int c = 0; c < KT; ++c) {
    const double* cs = a.cst + (size_t)b * 4 * KP + 16 * c + l16;
    ca[c] = model ? cs[0] : 0.0;
    cb[c] = model ? cs[KP] : 0.0;
    cc[c] = model ? cs[2 * KP] : 0.0;
    cw[c] = model ? cs[3 * KP] : 0.0;
  }
  d4 macc[KT][ETW];
#pragma unroll
  for (int c = 0; c < KT; ++c)
#pragma unroll
    for (int t = 0; t < ETW; ++t) macc[c][t] = d4{0.0, 0.0, 0.0, 0.0};

  const TS* ybase = static_cast<const TS*>(a.y) + (size_t)b * a.N * E;
  const int TPR = kWT / R;  // threads per row of the norm pass (4, 8 or 16)
  for (int64_t nb = n0; nb < n1; nb += R) {
    __syncthreads();  // the previous block's tile is no longer read
    const int rows = (int)((n1 - nb < R) ? n1 - nb : R);
    const TS* src = ybase + (size_t)nb * E;
    const int live = rows * E;
#pragma unroll 4
    for (int i = tid; i < R * E; i += kWT) {
      const int r = i / E, d = i - r * E;
      const TS raw = src[i < live ? i : 0];  // clamped, masked below
      ytile[r * LDY + d] = (i < live) ? (double)raw - gsh[d] : 0.0;
    }
    __syncthreads();
    {
      const int row = tid / TPR, j = tid - row * TPR;
      double q = 0.0;
      for (int d = j; d < E; d += TPR) {
        const double v = ytile[row * LDY + d];
        q = fma(v, v, q);
      }
      for (int m = 1; m < TPR; m <<= 1) q += __shfl_xor(q, m, kWave);
      if (j == 0) {
        const bool valid = row < rows;
        double sv = 0.0;
        if (valid) sv = a.sal ? a.sal[(size_t)b * a.N + nb + row] : 1.0;
        double one = 1.0, rs = 1.0, ms = 1.0;
        if (a.vmf) {
          // y_n / max(|y_n|, tiny) (vmfmm.py:76-78).  A row of zeros -- the padding rows of the
          // last block among them -- stays zero: scale 0, not 1 / tiny (kappa / tiny overflows,
          // and inf * 0 would poison the tile)
          const double nrm = sqrt(q);
          rs = nrm >= kTiny ? 1.0 / nrm : 0.0;
          if (a.mnorm && nrm >= kTiny) {
            one = nrm;
            ms = rs;
          }
        }
        ytile[row * LDY + E4] = valid ? one : 0.0;
        ytile[row * LDY + E4 + 1] = valid ? q : 0.0;
        rowaux[2 * row] = sv * ms;
        rowaux[2 * row + 1] = rs;
      }
    }
    __syncthreads();
    if (16 * wave >= R) continue;  // (barriers above are reached by every wavefront first)
    const int row0 = 16 * wave;
    double g[KT][4];
    if (model) {
      d4 acc[NM * KT];
#pragma unroll
      for (int c = 0; c < NM * KT; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
      if (a.mu_lds)
        wide_dots<NM * KT>(ytile, LDY, row0, mul, LDM, E4, lane, acc);
      else
        wide_dots<NM * KT>(ytile, LDY, row0, mug, E4, E4, lane, acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + 4 * r + lg;
        const int64_t n = nb + row;
        const bool valid = row < rows;
        const double q = ytile[row * LDY + E4 + 1];
        const double rs = rowaux[2 * row + 1];
        double lp[KT];
        if (DIAG) {
          double u2 = 0.0;
#pragma unroll
          for (int c = 0; c < KT; ++c) u2 = fma(acc[c][r], acc[c][r], u2);
          u2 = row16_sum(u2);
#pragma unroll
          for (int c = 0; c < KT; ++c) lp[c] = cb[c] + acc[KT + c][r] - 0.5 * u2;
        } else {
#pragma unroll
          for (int c = 0; c < KT; ++c) lp[c] = fma(ca[c], acc[c][r] * rs, fma(cc[c], q, cb[c]));
        }
        if (a.out_lp && valid) {
#pragma unroll
          for (int c = 0; c < KT; ++c)
            if (16 * c + l16 < K)
              a.out_lp[aff_index(b, 16 * c + l16, n, K, a.N, a.Tin)] = a.out_scale * lp[c];
        }
        if (!DIAG) {  // mixture_model_utils.py:30-47, affiliation_eps = 0
          double mx = lp[0];
#pragma unroll
          for (int c = 1; c < KT; ++c) mx = fmax(mx, lp[c]);
          mx = row16_max(mx);
          double den = 0.0;
#pragma unroll
          for (int c = 0; c < KT; ++c) {
            g[c][r] = exp(lp[c] - mx) * cw[c];
            den += g[c][r];
          }
          den = fmax(row16_sum(den), kTiny);
#pragma unroll
          for (int c = 0; c < KT; ++c) g[c][r] = g[c][r] / den;
          if (a.out_aff && valid) {
#pragma unroll
            for (int c = 0; c < KT; ++c)
              if (16 * c + l16 < K)
                a.out_aff[aff_index(b, 16 * c + l16, n, K, a.N, a.Tin)] = g[c][r];
          }
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t n = nb + row0 + 4 * r + lg;
#pragma unroll
        for (int c = 0; c < KT; ++c) {
          const int k = 16 * c + l16;
          g[c][r] = (k < K && n < n1) ? a.gamma[aff_index(b, k, n, K, a.N, a.Tin)] : 0.0;
        }
      }
    }
    if (!DIAG && a.accumulate) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double mw = rowaux[2 * (row0 + 4 * r + lg)];
#pragma unroll
        for (int c = 0; c < KT; ++c) g[c][r] *= mw;
      }
#pragma unroll
      for (int t = 0; t < ETW; ++t) {
        if (t < nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double bv = ytile[(row0 + 4 * r + lg) * LDY + 16 * (t0 + t) + l16];
            if (a.square) bv *= bv;
#pragma unroll
            for (int c = 0; c < KT; ++c)
              macc[c][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(g[c][r], bv, macc[c][t], 0, 0, 0);
          }
        }
      }
    }
  }
  if (DIAG || !a.accumulate) return;
  // the four wavefronts' tiles, added in wavefront order through LDS, then one chunk partial
  const int WC = 16 * nt;
  double* red = sm;
  for (int w = 0; w < kWT / kWave; ++w) {
    __syncthreads();
    if (wave == w && 16 * wave < R) {
#pragma unroll
      for (int c = 0; c < KT; ++c)
#pragma unroll
        for (int t = 0; t < ETW; ++t) {
          if (t < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int idx = (16 * c + 4 * r + lg) * WC + 16 * t + l16;
              red[idx] = (w == 0 ? 0.0 : red[idx]) + macc[c][t][r];
            }
          }
        }
    }
  }
  __syncthreads();
  double* dst = a.part + ((size_t)b * a.C + blockIdx.x) * K * a.EC;
  for (int i = tid; i < K * WC; i += kWT) {
    const int k = i / WC, j = i - k * WC;
    const int col = 16 * t0 + j;
    const int pc = col < E ? col : (col == E4 ? E : (col == E4 + 1 ? E + 1 : -1));
    if (pc >= 0) dst[(size_t)k * a.EC + pc] = red[i];
  }
}

// ---------------------------------------------------------------- finalize: one workgroup per class
// part / part2 (B, C, K, EC): columns [S1' (E) ; S0 ; S2'] of the sums about the shift.
//   vMF   (von_mises_fisher.py:122-144): mean direction, clipped concentration
//   'spherical' (gaussian.py:152-193): mean = g + S1' / den, variance about the mean from S2'
//   'diagonal': per-dimension variance from part2 (the sweep over the squares)
constexpr int kWideFinLoads = 8;
__global__ void __launch_bounds__(kWT)
    wide_finalize_kernel(int kind, const double* part, const double* part2, int C, int E, int E4,
                         int K, int EC, double cmin, double cmax, const double* shift,
                         double* out_mean, double* out_scale, double* s0raw) {
  extern __shared__ double sm[];  // tot [W2], red [nslot][W2]
  const int k = blockIdx.x;
  const int64_t b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int W2 = part2 ? 2 * EC : EC;
  double* tot = sm;
  double* red = sm + W2;
  const size_t cstride = (size_t)K * EC;
  const size_t base = ((size_t)b * C * K + k) * EC;
  if (W2 >= kWT) {
    for (int i = tid; i < W2; i += kWT) {
      const double* p = (i < EC ? part : part2) + base + (i < EC ? i : i - EC);
      double t = 0.0;
      for (int c = 0; c < C; ++c) t += p[c * cstride];
      tot[i] = t;
    }
  } else {
    const int nslot = kWT / W2;
    const int slot = tid / W2;
    const int i = tid - slot * W2;
    if (slot < nslot) {
      const double* p = (i < EC ? part : part2) + base + (i < EC ? i : i - EC);
      double t = 0.0;
      for (int c = slot; c < C; c += kWideFinLoads * nslot) {
        double v[kWideFinLoads];
#pragma unroll
        for (int u = 0; u < kWideFinLoads; ++u) {
          const int cc = c + u * nslot;
          v[u] = p[(cc < C ? cc : slot) * cstride];  // clamped, masked below
        }
#pragma unroll
        for (int u = 0; u < kWideFinLoads; ++u) t += (c + u * nslot < C) ? v[u] : 0.0;
      }
      red[slot * W2 + i] = t;
    }
    __syncthreads();
    for (int j = tid; j < W2; j += kWT) {
      double t = 0.0;
      for (int sl = 0; sl < nslot; ++sl) t += red[sl * W2 + j];
      tot[j] = t;
    }
  }
  __syncthreads();
  if (tid >= kWave) return;
  const double s0 = tot[E];
  double* mrow = out_mean + ((size_t)b * K + k) * E;
  if (lane == 0) s0raw[b * K + k] = s0;
  if (kind == PBBSS_EMBED_VMF) {
    double n2 = 0.0;
    for (int d = lane; d < E; d += kWave) n2 = fma(tot[d], tot[d], n2);
    n2 = wave_sum(n2);
    const double norm = sqrt(n2);
    const double rn = 1.0 / fmax(norm, kTiny);  // Banerjee 2005 eq. 2.4
    for (int d = lane; d < E; d += kWave) mrow[d] = tot[d] * rn;
    const double rbar = norm / s0;                                         // eq. 2.5
    double conc = (rbar * E - rbar * rbar * rbar) / (1.0 - rbar * rbar);  // eq. 4.4
    conc = conc < cmin ? cmin : (conc > cmax ? cmax : conc);              // NaN stays NaN
    if (lane == 0) out_scale[b * K + k] = conc;
    return;
  }
  // sum_n w (y - mean)^2 = S2' - 2 m' S1' + m'^2 S0 per dimension, m' = mean - g = S1' / den
  const double den = fmax(s0, kTiny);  // gaussian.py:160-163
  const double* g = shift + (size_t)b * E4;
  double cross = 0.0;
  for (int d = lane; d < E; d += kWave) {
    const double m = tot[d] / den;
    mrow[d] = g[d] + m;
    const double corr = m * (m * s0 - 2.0 * tot[d]);
    if (kind == PBBSS_EMBED_GAUSS_DIAG)
      out_scale[((size_t)b * K + k) * E + d] = (tot[EC + d] + corr) / den;  // gaussian.py:176-179
    cross += corr;
  }
  if (kind == PBBSS_EMBED_GAUSS_DIAG) return;
  cross = wave_sum(cross);
  if (lane == 0) out_scale[b * K + k] = (tot[E + 1] + cross) / (den * (double)E);  // :179-182
}

// ---------------------------------------------------------------- the model a sweep reads
// Padded class rows m' = mean - g (KP rows of E4, zeros beyond K and E) and per class the
// constants of  lp = a rs (y'.m') + c |y'|^2 + b:
//   vMF   a = kappa, c = 0, b = -log_norm(kappa), rs = 1 / |y_n|   (von_mises_fisher.py:33-44, :71-77)
//   Gauss a = 1 / cov, c = -1 / (2 cov), b = -E/2 ln 2pi + E ln(1 / sqrt(cov)) - |m'|^2 / (2 cov)
// and the mixture weights (mixture_model_utils.py:133-203): weight_mode 0 the L1-normalised
// weight sums of the finalize, 1 uniform, < 0 as given in `weight` (null: ones).
__global__ void __launch_bounds__(kWT)
    wide_model_kernel(int kind, int E, int E4, int K, int KP, const double* mean,
                      const double* scale, const double* shift, const double* s0raw,
                      int weight_mode, double* weight, double* mup, double* cst) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  double* cs = cst + (size_t)b * 4 * KP;
  // one wavefront per class, four classes per workgroup (gridDim.y = KP / 4): one workgroup
  // walking K / 4 classes in turn took 21 - 70 us at K = 64
  {
    const int k = blockIdx.y * (kWT / kWave) + wave;
    double* row = mup + ((size_t)b * KP + k) * E4;
    double ak = 0.0, bk = kNoClass, ck = 0.0;
    if (k < K) {
      double n2 = 0.0;
      for (int d = lane; d < E4; d += kWave) {
        double v = 0.0;
        if (d < E) v = mean[((size_t)b * K + k) * E + d] - (shift ? shift[(size_t)b * E4 + d] : 0.0);
        row[d] = v;
        n2 = fma(v, v, n2);
      }
      n2 = wave_sum(n2);
      const double sc = scale[b * K + k];
      if (kind == PBBSS_EMBED_VMF) {
        ak = sc;
        bk = -(0.5 * E * kLn2Pi + wave_log_bessel_over_power(0.5 * E - 1.0, sc, lane));
      } else {
        const double pc = 1.0 / sqrt(sc);  // sklearn _compute_precision_cholesky, 'diag' branch
        ak = pc * pc;
        ck = -0.5 * ak;
        bk = -0.5 * E * kLn2Pi + (double)E * log(pc) - 0.5 * ak * n2;
      }
    } else {
      for (int d = lane; d < E4; d += kWave) row[d] = 0.0;
    }
    if (lane == 0) {
      cs[k] = ak;
      cs[KP + k] = bk;
      cs[2 * KP + k] = ck;
    }
  }
  if (lane == 0) {
    const int tid = blockIdx.y * (kWT / kWave) + wave;  // this wavefront's class
    double w = 0.0;
    if (tid < K) {
      if (weight_mode == 1) {
        w = 1.0 / K;
      } else if (weight_mode == 0) {
        // estimate_mixture_weight with saliency: L1 unit norm over classes, eps 'where' 1e-10
        double t = 0.0;
        for (int k = 0; k < K; ++k) t += fabs(s0raw[b * K + k]);
        if (t == 0.0) t = 1e-10;
        w = s0raw[b * K + tid] / t;
      } else {
        w = weight ? weight[b * K + tid] : 1.0;
      }
      if (weight_mode >= 0) weight[b * K + tid] = w;
    }
    cs[3 * KP + tid] = w;
  }
}

// DiagonalGaussian.log_pdf AS WRITTEN in the reference (gaussian.py:76-97, see embed.hip): with
// pc = 1 / sqrt(cov) (K, E) used as ONE matrix, u_j(n) = pc_j . y'_n and c[j, k] = pc_j . m'_k,
//   log_pdf[k, n] = off_k - 1/2 sum_j (u_j(n) - c[j, k])^2
//                 = off_k - 1/2 |c_k|^2 + y'_n . v_k - 1/2 sum_j u_j(n)^2,   v_k = sum_j c[j, k] pc_j.
// Class rows: pc_j (first KP rows) and v_k (second KP rows); cst b = off_k - |c_k|^2 / 2.
__global__ void __launch_bounds__(kWT)
    wide_diag_model_kernel(int E, int E4, int K, int KP, const double* mean, const double* cov,
                           const double* shift, double* mup, double* cst) {
  extern __shared__ double cm[];  // [K][K]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  for (int i = tid; i < KP * E4; i += kWT) {
    const int j = i / E4, d = i - j * E4;
    mup[i] = (j < K && d < E) ? 1.0 / sqrt(cov[j * E + d]) : 0.0;
  }
  __syncthreads();
  for (int i = wave; i < K * K; i += kWT / kWave) {
    const int j = i / K, k = i - j * K;
    double t = 0.0;
    for (int e = lane; e < E; e += kWave) t = fma(mup[j * E4 + e], mean[k * E + e] - shift[e], t);
    t = wave_sum(t);
    if (lane == 0) cm[j * K + k] = t;
  }
  __syncthreads();
  for (int i = tid; i < KP * E4; i += kWT) {
    const int k = i / E4, e = i - k * E4;
    double v = 0.0;
    if (k < K && e < E)
      for (int j = 0; j < K; ++j) v = fma(mup[j * E4 + e], cm[j * K + k], v);
    mup[(size_t)KP * E4 + i] = v;
  }
  for (int k = wave; k < KP; k += kWT / kWave) {
    double bk = kNoClass;
    if (k < K) {
      double t = 0.0, c2 = 0.0;
      for (int e = lane; e < E; e += kWave) t += -0.5 * log(cov[k * E + e]);  // ln(1 / sqrt(cov))
      for (int j = lane; j < K; j += kWave) c2 = fma(cm[j * K + k], cm[j * K + k], c2);
      t = wave_sum(t);
      c2 = wave_sum(c2);
      bk = -0.5 * E * kLn2Pi + t - 0.5 * c2;
    }
    if (lane == 0) {
      cst[k] = 0.0;
      cst[KP + k] = bk;
      cst[2 * KP + k] = 0.0;
      cst[3 * KP + k] = 1.0;
    }
  }
}

// g = column mean of every mixture (unweighted: one g serves all classes and iterations), padded
// to E4.  Stage 1, grid (C, B): thread t adds column t % E over the rows r, r + RL, ... of the
// chunk (r = t / E, RL = 256 / E row lanes), the row lanes are added in order:
// part[(b C + c) E + d], bit-reproducible.  Stage 2, one workgroup per mixture: chunks in order.
static_assert(kEmbedMaxE <= kWT, "one thread per column");
__global__ void __launch_bounds__(kWT)
    wide_shift_part_kernel(const void* y, int y_is_f64, int64_t N, int E, int64_t L, double* part) {
  __shared__ double red[kWT];
  const int c = blockIdx.x, C = gridDim.x, tid = threadIdx.x;
  const int64_t b = blockIdx.y;
  const int RL = kWT / E, d = tid % E, r = tid / E;
  const int64_t n0 = (int64_t)c * L;
  const int64_t n1 = (n0 + L < N) ? n0 + L : N;
  const size_t base = (size_t)b * N * E + d;
  auto at = [&](int64_t n) {
    return y_is_f64 ? static_cast<const double*>(y)[base + (size_t)n * E]
                    : (double)static_cast<const float*>(y)[base + (size_t)n * E];
  };
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  if (r < RL) {
    int64_t n = n0 + r;
    for (; n + 3 * (int64_t)RL < n1; n += 4 * (int64_t)RL) {
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = at(n + (int64_t)u * RL);
#pragma unroll
      for (int u = 0; u < 4; ++u) t[u] += v[u];
    }
    for (; n < n1; n += RL) t[0] += at(n);
  }
  red[tid] = (t[0] + t[1]) + (t[2] + t[3]);
  __syncthreads();
  if (tid < E) {
    double v = 0.0;
    for (int q = 0; q < RL; ++q) v += red[q * E + tid];
    part[((size_t)b * C + c) * E + tid] = v;
  }
}
__global__ void wide_shift_kernel(const double* part, int C, int64_t N, int E, int E4,
                                  double* shift) {
  const int64_t b = blockIdx.x;
  for (int d = threadIdx.x; d < E4; d += blockDim.x) {
    double v = 0.0;
    if (d < E) {
      for (int c = 0; c < C; ++c) v += part[((size_t)b * C + c) * E + d];
      v /= (double)N;
    }
    shift[(size_t)b * E4 + d] = v;
  }
}

// ---------------------------------------------------------------- joint-model class weights
// (gcacgmm.py:286-295) for any K <= 64; modes and scratch as launch_joint_weight in embed.hip.
// modes 0 / 2: workgroup f, one wavefront per class in turn: sum_t aff[f,k,t] sal[f,t] -> tmp[f,k]
// (mode 0: normalised over the classes into out[f,k])
__global__ void __launch_bounds__(kWT)
    wide_rowsum_kernel(const double* aff, const double* sal, int K, int T, int normalize,
                       double* tmp, double* out) {
  __shared__ double v[kEmbedWideMaxK];
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  for (int k = wave; k < K; k += kWT / kWave) {
    double t = 0.0;
    for (int i = lane; i < T; i += kWave)
      t += aff[((size_t)f * K + k) * T + i] * (sal ? sal[(size_t)f * T + i] : 1.0);
    t = wave_sum(t);
    if (lane == 0) v[k] = t;
  }
  __syncthreads();
  if (tid < K) {
    double tot = 0.0;
    for (int k = 0; k < K; ++k) tot += v[k];
    if (normalize) out[f * K + tid] = v[tid] / tot;  // gcacgmm.py:292-294
    else tmp[f * K + tid] = v[tid];
  }
}
// mode 2: single workgroup, thread k adds the row sums of class k over the bins in order
__global__ void __launch_bounds__(kWT)
    wide_rows_to_class_kernel(const double* tmp, int64_t F, int K, double* out) {
  __shared__ double v[kEmbedWideMaxK];
  const int tid = threadIdx.x;
  if (tid < K) {
    double t = 0.0;
    for (int64_t f = 0; f < F; ++f) t += tmp[f * K + tid];
    v[tid] = t;
  }
  __syncthreads();
  if (tid < K) {
    double tot = 0.0;
    for (int k = 0; k < K; ++k) tot += v[k];
    out[tid] = v[tid] / tot;
  }
}
// mode 3: slice sums over the bins -> part (slice, K, T), then added in slice order and
// normalised over the classes per frame
__global__ void __launch_bounds__(kWT)
    wide_colsum_part_kernel(const double* aff, const double* sal, int64_t F, int K, int T,
                            double* part) {
  const int t = blockIdx.x * kWT + threadIdx.x;
  if (t >= T) return;
  const int64_t per = (F + gridDim.y - 1) / gridDim.y;
  const int64_t f0 = per * blockIdx.y;
  const int64_t f1 = f0 + per < F ? f0 + per : F;
  for (int k = 0; k < K; ++k) {
    double sk = 0.0;
    for (int64_t f = f0; f < f1; ++f)
      sk += aff[((size_t)f * K + k) * T + t] * (sal ? sal[(size_t)f * T + t] : 1.0);
    part[((size_t)blockIdx.y * K + k) * T + t] = sk;
  }
}
__global__ void __launch_bounds__(kWT)
    wide_colsum_fin_kernel(const double* part, int slices, int K, int T, double* out) {
  const int t = blockIdx.x * kWT + threadIdx.x;
  if (t >= T) return;
  double tot = 0.0;
  for (int k = 0; k < K; ++k) {
    double vk = 0.0;
    for (int c = 0; c < slices; ++c) vk += part[((size_t)c * K + k) * T + t];
    out[(size_t)k * T + t] = vk;
    tot += vk;
  }
  for (int k = 0; k < K; ++k) out[(size_t)k * T + t] /= tot;
}
__global__ void wide_fill_kernel(double* out, double v) { out[0] = v; }

inline int ok_or_hip() { return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP; }

// ---------------------------------------------------------------- host: plan and workspace
struct WidePlan {
  int KT, KP, E4, ET, ETW, FS, LDY, R, C, EC, ybuf;
  int64_t L;
};

WidePlan wide_plan(int64_t B, int64_t N, int E, int K) {
  WidePlan p;
  p.KT = (K + 15) / 16;
  p.KP = 16 * p.KT;
  p.E4 = (E + 3) & ~3;
  p.ET = (p.E4 + 2 + 15) / 16;  // column tiles of [y' ; 1 ; |y'|^2]
  p.ETW = 16 / p.KT;  // up to 64 accumulator doubles a lane; four tiles (E <= 60) need fewer
  if (p.ET <= 4 && p.ETW > 4) p.ETW = 4;
  p.FS = (p.ET + p.ETW - 1) / p.ETW;
  p.LDY = 16 * p.ET + 1;
  p.R = 64 * p.LDY <= 4608 ? 64 : (32 * p.LDY <= 4608 ? 32 : 16);  // row tile <= 36 KiB
  const int red = p.KP * 16 * (p.ET < p.ETW ? p.ET : p.ETW);
  p.ybuf = p.R * p.LDY > red ? p.R * p.LDY : red;
  p.EC = E + 2;
  const int64_t blocks = (N + p.R - 1) / p.R;
  int64_t want = 512 / (B * p.FS);  // about two workgroups per compute unit in total
  if (want < 1) want = 1;
  const int64_t c0 = blocks < want ? blocks : want;
  p.L = (blocks + c0 - 1) / c0 * p.R;
  p.C = (int)((N + p.L - 1) / p.L);
  return p;
}

struct WideWork {
  double *part, *part2, *mup, *cst, *s0, *shift;
};
size_t wide_carve(double* base, int64_t B, const WidePlan& p, int K, WideWork* w) {
  size_t off = 0;
  auto take = [&](size_t n) {
    double* q = base ? base + off : nullptr;
    off += (n + 31) & ~(size_t)31;
    return q;
  };
  const size_t np = (size_t)B * p.C * K * p.EC;
  WideWork ww;
  ww.part = take(np);
  ww.part2 = take(np);
  ww.mup = take((size_t)B * 2 * p.KP * p.E4);
  ww.cst = take((size_t)B * 4 * p.KP);
  ww.s0 = take((size_t)B * K);
  ww.shift = take((size_t)B * p.E4);
  if (w) *w = ww;
  return off;
}

bool wide_shape_ok(int64_t B, int64_t N, int E, int K) {
  return B >= 1 && B <= 65535 && N >= 1 && E >= 1 && E <= kEmbedMaxE && K >= 1 &&
         K <= kEmbedWideMaxK;
}

struct Sweep {
  int kind, y_is_f64, nm;
  const void* y;
  int64_t B, N, Tin;
  int E, K;
  const double *gamma, *sal;
  int mnorm, square, accumulate;
  double out_scale;
  double *out_lp, *out_aff, *part;
};

template <typename TS, int KT>
int sweep_go(const SweepArgs& a, int nm, int etw, dim3 grid, size_t lds, hipStream_t s) {
  constexpr int kFull = 16 / KT;
  if (nm == 2)
    hipLaunchKernelGGL((wide_sweep_kernel<TS, KT, 2, 1>), grid, dim3(kWT), lds, s, a);
  else if (etw == kFull)
    hipLaunchKernelGGL((wide_sweep_kernel<TS, KT, 1, kFull>), grid, dim3(kWT), lds, s, a);
  else
    hipLaunchKernelGGL((wide_sweep_kernel<TS, KT, 1, (kFull < 4 ? kFull : 4)>), grid, dim3(kWT), lds,
                       s, a);
  return ok_or_hip();
}

int launch_wide_sweep(const Sweep& q, const WidePlan& p, const WideWork& w, size_t lds_limit,
                      hipStream_t s) {
  SweepArgs a;
  a.y = q.y;
  a.N = q.N;
  a.L = p.L;
  a.Tin = q.Tin;
  a.E = q.E;
  a.E4 = p.E4;
  a.K = q.K;
  a.R = p.R;
  a.LDY = p.LDY;
  a.ET = p.ET;
  a.C = p.C;
  a.EC = p.EC;
  a.ybuf = p.ybuf;
  a.gamma = q.gamma;
  a.sal = q.sal;
  a.vmf = q.kind == PBBSS_EMBED_VMF;
  a.shift = a.vmf ? nullptr : w.shift;
  a.mnorm = q.mnorm;
  a.square = q.square;
  a.accumulate = q.accumulate;
  a.mup = w.mup;
  a.cst = w.cst;
  a.out_scale = q.out_scale;
  a.out_lp = q.out_lp;
  a.out_aff = q.out_aff;
  a.part = q.part;
  // class rows in LDS where they fit into what a launch gets without an attribute (64 KiB)
  const size_t limit = lds_limit < 65536 ? lds_limit : 65536;
  const size_t fixed = ((size_t)p.ybuf + 2 * p.R + p.E4) * sizeof(double);
  const size_t mu = q.gamma ? 0 : (size_t)q.nm * p.KP * (p.E4 + 1) * sizeof(double);
  if (fixed > limit) return PBBSS_ERR_UNSUPPORTED;
  a.mu_lds = fixed + mu <= limit;
  const size_t lds = fixed + (a.mu_lds ? mu : 0);
  dim3 grid((unsigned)p.C, (unsigned)q.B, (unsigned)(q.accumulate ? p.FS : 1));
  return dispatch_range<1, 4>(p.KT, [&](auto kt) {
    return dispatch_real(q.y_is_f64, [&](auto ys) {
      return sweep_go<decltype(ys), kt()>(a, q.nm, p.ETW, grid, lds, s);
    });
  });
}

int launch_wide_finalize(int kind, int64_t B, int E, int K, const WidePlan& p, const WideWork& w,
                         bool second, double cmin, double cmax, double* out_mean,
                         double* out_scale, hipStream_t s) {
  const int W2 = second ? 2 * p.EC : p.EC;
  const size_t lds = ((size_t)W2 + (W2 < kWT ? (size_t)(kWT / W2) * W2 : 0)) * sizeof(double);
  hipLaunchKernelGGL(wide_finalize_kernel, dim3((unsigned)K, (unsigned)B), dim3(kWT), lds, s, kind,
                     w.part, second ? w.part2 : nullptr, p.C, E, p.E4, K, p.EC, cmin, cmax, w.shift,
                     out_mean, out_scale, w.s0);
  return ok_or_hip();
}

int launch_wide_model(int kind, int64_t B, int E, int K, const WidePlan& p, const WideWork& w,
                      const double* mean, const double* scale, bool from_sums, int weight_mode,
                      double* weight, hipStream_t s) {
  hipLaunchKernelGGL(wide_model_kernel, dim3((unsigned)B, (unsigned)(p.KP / 4)), dim3(kWT), 0, s, kind, E, p.E4, K, p.KP,
                     mean, scale, kind == PBBSS_EMBED_VMF ? nullptr : w.shift,
                     from_sums ? w.s0 : nullptr, weight_mode, weight, w.mup, w.cst);
  return ok_or_hip();
}

int launch_wide_shift(int kind, const void* y, int y_is_f64, int64_t B, int64_t N, int E,
                      const WidePlan& p, const WideWork& w, hipStream_t s) {
  if (kind == PBBSS_EMBED_VMF) return PBBSS_OK;
  // the chunk sums (B, C, E) borrow the head of the sweep partials (B, C, K, EC): no sweep has
  // run yet when the shift is taken
  hipLaunchKernelGGL(wide_shift_part_kernel, dim3((unsigned)p.C, (unsigned)B), dim3(kWT), 0, s, y,
                     y_is_f64, N, E, p.L, w.part);
  hipLaunchKernelGGL(wide_shift_kernel, dim3((unsigned)B), dim3(kWT), 0, s, w.part, p.C, N, E,
                     p.E4, w.shift);
  return ok_or_hip();
}

}  // namespace

size_t embed_wide_work_doubles(int64_t B, int64_t N, int E, int K) {
  if (!wide_shape_ok(B, N, E, K)) return 0;
  return wide_carve(nullptr, B, wide_plan(B, N, E, K), K, nullptr);
}

int embed_wide_mixture(int kind, const void* y, int y_is_f64, int64_t B, int64_t N, int E, int K,
                       const double* gamma0, const double* saliency, const double* fixed_scale,
                       int iterations, int weight_mode, double cmin, double cmax, double* work,
                       double* out_mean, double* out_scale, double* out_weight, double* out_aff,
                       double* out_lp, size_t lds_limit, hipStream_t s) {
  if (!wide_shape_ok(B, N, E, K)) return PBBSS_ERR_UNSUPPORTED;
  if (kind != PBBSS_EMBED_VMF && kind != PBBSS_EMBED_GAUSS_SPHERICAL) return PBBSS_ERR_UNSUPPORTED;
  const WidePlan p = wide_plan(B, N, E, K);
  WideWork w;
  wide_carve(work, B, p, K, &w);
  const bool vmf = kind == PBBSS_EMBED_VMF;
  int rc = launch_wide_shift(kind, y, y_is_f64, B, N, E, p, w, s);
  if (rc != PBBSS_OK) return rc;
  Sweep q{};
  q.kind = kind;
  q.y_is_f64 = y_is_f64;
  q.nm = 1;
  q.y = y;
  q.B = B;
  q.N = N;
  q.Tin = N;
  q.E = E;
  q.K = K;
  q.mnorm = vmf;  // the vMF mixture works on unit rows (vmfmm.py:76-78)
  q.out_scale = 1.0;
  if (iterations == 0) {  // the caller's model: weights as given
    rc = launch_wide_model(kind, B, E, K, p, w, out_mean, out_scale, false, -1, out_weight, s);
    if (rc != PBBSS_OK) return rc;
  }
  for (int it = 0; it < iterations; ++it) {
    // vmfmm.py:131-172 / gmm.py:126-171: E-step with the previous model (the initialisation in
    // the first iteration), M-step from the same rows
    q.gamma = it == 0 ? gamma0 : nullptr;
    q.sal = saliency;
    q.accumulate = 1;
    q.part = w.part;
    if ((rc = launch_wide_sweep(q, p, w, lds_limit, s)) != PBBSS_OK) return rc;
    rc = launch_wide_finalize(kind, B, E, K, p, w, false, cmin, cmax, out_mean, out_scale, s);
    if (rc != PBBSS_OK) return rc;
    if (fixed_scale) {  // gmm.py:160-167
      if (hipMemcpyAsync(out_scale, fixed_scale, (size_t)B * K * 8, hipMemcpyDeviceToDevice, s) !=
          hipSuccess)
        return PBBSS_ERR_HIP;
    }
    rc = launch_wide_model(kind, B, E, K, p, w, out_mean, out_scale, true, weight_mode, out_weight, s);
    if (rc != PBBSS_OK) return rc;
  }
  if (out_aff || out_lp) {
    q.gamma = nullptr;
    q.sal = nullptr;
    q.accumulate = 0;
    q.part = nullptr;
    q.out_aff = out_aff;
    q.out_lp = out_lp;
    if ((rc = launch_wide_sweep(q, p, w, lds_limit, s)) != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}

int embed_wide_fit(int kind, const void* y, int y_is_f64, int64_t B, int64_t N, int E, int K,
                   const double* weights, int normalize, double cmin, double cmax, double* work,
                   double* out_mean, double* out_scale, size_t lds_limit, hipStream_t s,
                   int64_t Tin, const double* sal, bool have_shift) {
  if (!wide_shape_ok(B, N, E, K)) return PBBSS_ERR_UNSUPPORTED;
  if (kind != PBBSS_EMBED_VMF && kind != PBBSS_EMBED_GAUSS_SPHERICAL && kind != PBBSS_EMBED_GAUSS_DIAG)
    return PBBSS_ERR_UNSUPPORTED;
  const WidePlan p = wide_plan(B, N, E, K);
  WideWork w;
  wide_carve(work, B, p, K, &w);
  int rc = have_shift ? PBBSS_OK : launch_wide_shift(kind, y, y_is_f64, B, N, E, p, w, s);
  if (rc != PBBSS_OK) return rc;
  Sweep q{};
  q.kind = kind;
  q.y_is_f64 = y_is_f64;
  q.nm = 1;
  q.y = y;
  q.B = B;
  q.N = N;
  q.Tin = Tin > 0 ? Tin : N;
  q.E = E;
  q.K = K;
  q.gamma = weights;
  q.sal = sal;
  q.mnorm = kind == PBBSS_EMBED_VMF && normalize;
  q.accumulate = 1;
  q.out_scale = 1.0;
  q.part = w.part;
  if ((rc = launch_wide_sweep(q, p, w, lds_limit, s)) != PBBSS_OK) return rc;
  const bool diag = kind == PBBSS_EMBED_GAUSS_DIAG;
  if (diag) {  // per-dimension second moments about the shift: the same sweep over the squares
    q.square = 1;
    q.part = w.part2;
    if ((rc = launch_wide_sweep(q, p, w, lds_limit, s)) != PBBSS_OK) return rc;
  }
  return launch_wide_finalize(kind, B, E, K, p, w, diag, cmin, cmax, out_mean, out_scale, s);
}

int embed_wide_shift(int kind, const void* y, int y_is_f64, int64_t B, int64_t N, int E, int K,
                     double* work, hipStream_t s) {
  if (!wide_shape_ok(B, N, E, K)) return PBBSS_ERR_UNSUPPORTED;
  const WidePlan p = wide_plan(B, N, E, K);
  WideWork w;
  wide_carve(work, B, p, K, &w);
  return launch_wide_shift(kind, y, y_is_f64, B, N, E, p, w, s);
}

int embed_wide_joint_weight(int mode, const double* aff, const double* sal, int64_t F, int K, int T,
                            double* tmp, double* out_weight, hipStream_t s) {
  if (K < 1 || K > kEmbedWideMaxK || F > 2147483647LL) return PBBSS_ERR_UNSUPPORTED;
  switch (mode) {
    case 0:
      hipLaunchKernelGGL(wide_rowsum_kernel, dim3((unsigned)F), dim3(kWT), 0, s, aff, sal, K, T, 1,
                         tmp, out_weight);
      break;
    case 1:
      hipLaunchKernelGGL(wide_fill_kernel, dim3(1), dim3(1), 0, s, out_weight, 1.0 / K);
      break;
    case 2:
      hipLaunchKernelGGL(wide_rowsum_kernel, dim3((unsigned)F), dim3(kWT), 0, s, aff, sal, K, T, 0,
                         tmp, out_weight);
      hipLaunchKernelGGL(wide_rows_to_class_kernel, dim3(1), dim3(kWT), 0, s, tmp, F, K,
                         out_weight);
      break;
    case 3: {
      // as many bin slices as joint_weight_tmp_doubles(3, ...) leaves room for
      const int slices = (int)(joint_weight_tmp_doubles(3, F, K, T) / ((size_t)K * T));
      const unsigned gx = (unsigned)((T + kWT - 1) / kWT);
      hipLaunchKernelGGL(wide_colsum_part_kernel, dim3(gx, (unsigned)slices), dim3(kWT), 0, s, aff,
                         sal, F, K, T, tmp);
      hipLaunchKernelGGL(wide_colsum_fin_kernel, dim3(gx), dim3(kWT), 0, s, tmp, slices, K, T,
                         out_weight);
      break;
    }
    case 4:
      hipLaunchKernelGGL(wide_fill_kernel, dim3(1), dim3(1), 0, s, out_weight, 1.0);
      break;
    default: return PBBSS_ERR_INVALID_ARG;
  }
  return ok_or_hip();
}

int embed_wide_log_pdf(int kind, const void* y, int y_is_f64, int64_t B, int64_t N, int E, int K,
                       const double* mean, const double* scale, double out_scale, int64_t Tin,
                       double* work, double* out_lp, size_t lds_limit, hipStream_t s,
                       bool have_shift) {
  if (!wide_shape_ok(B, N, E, K)) return PBBSS_ERR_UNSUPPORTED;
  const WidePlan p = wide_plan(B, N, E, K);
  WideWork w;
  wide_carve(work, B, p, K, &w);
  int rc = have_shift ? PBBSS_OK : launch_wide_shift(kind, y, y_is_f64, B, N, E, p, w, s);
  if (rc != PBBSS_OK) return rc;
  Sweep q{};
  q.kind = kind;
  q.y_is_f64 = y_is_f64;
  q.nm = 1;
  q.y = y;
  q.B = B;
  q.N = N;
  q.Tin = Tin;
  q.E = E;
  q.K = K;
  q.out_scale = out_scale;
  q.out_lp = out_lp;
  if (kind == PBBSS_EMBED_GAUSS_DIAG) {
    if (B != 1) return PBBSS_ERR_UNSUPPORTED;  // the reference's DiagonalGaussian has no batch axis
    q.nm = 2;
    hipLaunchKernelGGL(wide_diag_model_kernel, dim3(1), dim3(kWT), (size_t)K * K * sizeof(double), s,
                       E, p.E4, K, p.KP, mean, scale, w.shift, w.mup, w.cst);
    if ((rc = ok_or_hip()) != PBBSS_OK) return rc;
  } else if (kind == PBBSS_EMBED_VMF || kind == PBBSS_EMBED_GAUSS_SPHERICAL) {
    rc = launch_wide_model(kind, B, E, K, p, w, mean, scale, false, -1, nullptr, s);
    if (rc != PBBSS_OK) return rc;
  } else {
    return PBBSS_ERR_UNSUPPORTED;
  }
  return launch_wide_sweep(q, p, w, lds_limit, s);
}

}  // namespace pbbss
