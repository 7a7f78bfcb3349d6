// WPE dereverberation (include/pbbss.h, XIII; nara_wpe.wpe: get_power_inverse, get_correlations,
// get_filter_matrix, perform_filter_operation, wpe) on frames read through the caller's strides.
//
// power:        one thread per frame: the mean of |y|^2 over the sensors.
// weights:      one workgroup per problem: the smoothing over psd_context frames (window sums in
//               ascending order; all frames: a fixed tree), the row maximum and
//               1 / max(power, 1e-10 max).  A row that is all zero gets weight 0 (not 1 / 0) and
//               its maximum tells the solver to leave the problem alone.
// correlations: one workgroup per (problem, span of kWpeSpan frames).  The stacked vector is never
//               materialised: the span's frames and the taps - 1 + span frames `delay` behind
//               them lie in LDS once, tap k of sensor d is the second array shifted by k.  The
//               Gram matrix of the extended vector (ytilde ; y), M + D rows, holds R (top left)
//               and P^H (bottom left); its lower block triangle is summed on
//               v_mfma_f64_16x16x4_f64 tiles: a k-step is two frames times (re, im), lane l
//               feeds A[i = l % 16][k = l / 16] and B[k = l / 16][j = l % 16] and holds
//               D[4 r + l / 16][l % 16] in accumulator register r (as gauss_full.hip).  With
//               z = a + i b:  Re z_i conj(z_j) = a_i a_j + b_i b_j,  Im = b_i a_j - a_i b_j, so
//               the real tile takes A = w (a_i, b_i), the imaginary one A = w (b_i, -a_i), both
//               B = (a_j, b_j).  Every workgroup writes its span sums; a second kernel adds the
//               spans in ascending order, mirrors R and transposes P.  No atomics; the spans do
//               not depend on the number of problems.
// solve:        one workgroup per problem: the lower triangle of R packed in LDS, right-looking
//               Cholesky (all threads share the trailing update), forward and backward
//               substitution on the D columns of P, a status word.
// apply:        one thread per frame: x_t = y_t - G^H ytilde_t with G and the shifted frames in
//               LDS, D accumulators in registers; the same pass writes the power of x for the
//               next iteration's weights.
#include "wpe.hpp"
#include <math.h>
#include "dispatch.hpp"
#include "frame_tile.hpp"
#include "launch_util.hpp"

namespace pbbss {
namespace {

constexpr int kThreads = 256;
typedef double double4_t __attribute__((ext_vector_type(4)));

// frames f0 .. f0 + W - 1 of every sensor of problem b to dst[d * WS + u]; frames outside the row
// are zeros.  The inner index of the copy is the axis that is contiguous in memory.
__device__ __forceinline__ void stage_rows(const WpeFrames& y, int64_t b, int64_t f0, int W, int WS,
                                           double2* dst, int tid) {
  const int D = y.D, n = D * W;
  const bool d_inner = y.sd == 1 && D > 1;
  for (int idx = tid; idx < n; idx += kThreads) {
    int d, u;
    if (d_inner) {
      u = idx / D;
      d = idx - u * D;
    } else {
      d = idx / W;
      u = idx - d * W;
    }
    const int64_t f = f0 + u;
    double2 v = make_double2(0.0, 0.0);
    if (f >= 0 && f < y.T) v = load_frame(y, b * y.sb + d * y.sd + f * y.st);
    dst[d * WS + u] = v;
  }
}

// ---------------------------------------------------------------------------------------- power
__global__ __launch_bounds__(kThreads) void wpe_power_kernel(WpeFrames y, int tiles, double* raw) {
  const int64_t b = blockIdx.x / tiles;
  const int64_t t = (int64_t)(blockIdx.x - b * tiles) * kThreads + threadIdx.x;
  if (t >= y.T) return;
  double s = 0.0;
  for (int d = 0; d < y.D; ++d) {
    const double2 v = load_frame(y, b * y.sb + d * y.sd + t * y.st);
    s += v.x * v.x + v.y * v.y;
  }
  raw[b * y.T + t] = s / (double)y.D;
}

__global__ __launch_bounds__(kThreads) void wpe_weight_kernel(const double* raw, int64_t T,
                                                              int64_t ctx, double* out_power,
                                                              double* out_inv, double* out_pmax) {
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double* p = raw + b * T;
  double* q = out_power + b * T;
  double mean = 0.0;
  if (ctx < 0) {  // one value for the row: a fixed tree over interleaved slices
    double s = 0.0;
    for (int64_t t = tid; t < T; t += kThreads) s += p[t];
    red[tid] = s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
      if (tid < w) red[tid] += red[tid + w];
      __syncthreads();
    }
    mean = red[0] / (double)T;
    __syncthreads();
  }
  double m = 0.0;
  for (int64_t t = tid; t < T; t += kThreads) {
    double v;
    if (ctx < 0) {
      v = mean;
    } else if (ctx == 0) {
      v = p[t];
    } else {  // the frames of [t - ctx, t + ctx] that exist, in ascending order
      const int64_t lo = t - ctx < 0 ? 0 : t - ctx, hi = ctx >= T - t ? T - 1 : t + ctx;
      double s = 0.0;
      for (int64_t u = lo; u <= hi; ++u) s += p[u];
      v = s / (double)(hi - lo + 1);
    }
    q[t] = v;
    m = (v > m || v != v) ? v : m;  // a NaN stays, as in np.max
  }
  red[tid] = m;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
      const double o = red[tid + w];
      red[tid] = (o > red[tid] || o != o) ? o : red[tid];
    }
    __syncthreads();
  }
  const double qmax = red[0], fl = 1e-10 * qmax;
  if (tid == 0 && out_pmax) out_pmax[b] = qmax;
  if (!out_inv) return;
  for (int64_t t = tid; t < T; t += kThreads) {  // q[t] was written by this thread
    const double v = q[t];
    const double c = v >= fl ? v : (v != v ? v : fl);  // np.maximum: a NaN stays
    out_inv[b * T + t] = qmax == 0.0 ? 0.0 : 1.0 / c;
  }
}

// --------------------------------------------------------------------------------- correlations
// LDS: cur [D][kWpeSpan + 1] | past [D][(kWpeSpan + taps - 1) | 1] complex128 | weights [kWpeSpan]
// part[((b * spans + span) * tiles + q) * 256 + row * 16 + col], q = I (I + 1) / 2 + J the tile
// (I, J <= I) of the lower block triangle.
template <int TPW>
__global__ __launch_bounds__(kThreads) void wpe_corr_kernel(WpeFrames y, const double* inv,
                                                            int taps, int delay, int valid,
                                                            int spans, int tiles, double2* part) {
  extern __shared__ double2 wpe_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = y.D, M = D * taps, Me = M + D;
  const int SP = kWpeSpan + 1, WP = (kWpeSpan + taps - 1) | 1;
  const int64_t b = blockIdx.x / spans;
  const int span = (int)(blockIdx.x - b * spans);
  const int64_t t0 = (int64_t)span * kWpeSpan;
  const int nf = (int)(y.T - t0 < kWpeSpan ? y.T - t0 : kWpeSpan);
  double2* cur = wpe_lds;
  double2* past = cur + D * SP;
  double* lam = reinterpret_cast<double*>(past + D * WP);
  stage_rows(y, b, t0, kWpeSpan, SP, cur, tid);
  stage_rows(y, b, t0 - delay - taps + 1, kWpeSpan + taps - 1, WP, past, tid);
  for (int u = tid; u < kWpeSpan; u += kThreads) {
    const int64_t t = t0 + u;
    const bool use = u < nf && !(valid && t < (int64_t)delay + taps - 1);
    lam[u] = use ? inv[b * y.T + t] : 0.0;
  }
  __syncthreads();
  // row e of the extended vector at local frame tl: wpe_lds[row_off(e) + tl]
  auto row_off = [&](int e) {
    if (e >= Me) e = Me - 1;  // rows of the padding: read in bounds, never written out
    if (e >= M) return (e - M) * SP;
    const int k = e / D, d = e - k * D;
    return D * SP + d * WP + (taps - 1 - k);
  };
  int offI[TPW], offJ[TPW];
  double4_t accr[TPW], acci[TPW];
  int mine = 0;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int q = wave + 4 * i;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= q) ++I;
    const int J = q - I * (I + 1) / 2;
    offI[i] = row_off(kWpeTile * I + (lane & 15));
    offJ[i] = row_off(kWpeTile * J + (lane & 15));
    accr[i] = double4_t{0.0, 0.0, 0.0, 0.0};
    acci[i] = double4_t{0.0, 0.0, 0.0, 0.0};
    if (q < tiles) mine = i + 1;
  }
  const int kk = lane >> 4, im = kk & 1, fr = kk >> 1;
  const int steps = (nf + 1) >> 1;
  for (int ks = 0; ks < steps; ++ks) {
    const int tl = 2 * ks + fr;  // <= kWpeSpan - 1; a frame behind the row has weight 0
    const double w = lam[tl];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      if (i < mine) {
        const double2 zi = wpe_lds[offI[i] + tl];
        const double2 zj = wpe_lds[offJ[i] + tl];
        const double bj = im ? zj.y : zj.x;
        const double ar = w * (im ? zi.y : zi.x);
        const double ai = w * (im ? -zi.x : zi.y);
        accr[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bj, accr[i], 0, 0, 0);
        acci[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, bj, acci[i], 0, 0, 0);
      }
    }
  }
  double2* out = part + ((b * spans + span) * tiles) * 256;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    if (i < mine) {
      const int q = wave + 4 * i;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[q * 256 + (4 * r + kk) * kWpeTile + (lane & 15)] = make_double2(accr[i][r], acci[i][r]);
    }
  }
}

__global__ __launch_bounds__(kThreads) void wpe_corr_finish_kernel(const double2* part,
                                                                   int64_t total, int D, int taps,
                                                                   int spans, int tiles,
                                                                   double2* R, double2* P) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int M = D * taps, Me = M + D;
  const int64_t b = i / ((int64_t)tiles * 256);
  const int rem = (int)(i - b * tiles * 256);
  const int q = rem >> 8, e = rem & 255;
  int I = 0;
  while ((I + 1) * (I + 2) / 2 <= q) ++I;
  const int J = q - I * (I + 1) / 2;
  const int row = kWpeTile * I + (e >> 4), col = kWpeTile * J + (e & 15);
  if (row >= Me || col > row || col >= M) return;
  const double2* p = part + (b * spans * tiles + q) * 256 + e;
  double sr = 0.0, si = 0.0;
  for (int sp = 0; sp < spans; ++sp, p += (int64_t)tiles * 256) {
    sr += p->x;
    si += p->y;
  }
  if (row < M) {
    double2* Rb = R + b * M * M;
    if (row == col) {
      Rb[row * M + col] = make_double2(sr, 0.0);
    } else {
      Rb[row * M + col] = make_double2(sr, si);
      Rb[col * M + row] = make_double2(sr, -si);
    }
  } else {  // (y_d conj ytilde_m): the conjugate of P[m][d]
    P[(b * M + col) * D + (row - M)] = make_double2(sr, -si);
  }
}

// ---------------------------------------------------------------------------------------- solve
// LDS: L [M (M + 1) / 2] packed lower triangle | Z [M][D] complex128 | reciprocal diagonal [M]
__global__ __launch_bounds__(kThreads) void wpe_solve_kernel(const double2* R, const double2* P,
                                                             const double* pmax, int D, int taps,
                                                             double2* G, int32_t* status) {
  extern __shared__ double2 wpe_lds[];
  const int tid = threadIdx.x;
  const int M = D * taps, MD = M * D;
  const int64_t b = blockIdx.x;
  double2* L = wpe_lds;
  double2* Z = L + M * (M + 1) / 2;
  double* invd = reinterpret_cast<double*>(Z + MD);
  double2* Gb = G + b * MD;
  if (pmax && pmax[b] == 0.0) {  // an all-zero problem: nothing to predict
    for (int e = tid; e < MD; e += kThreads) Gb[e] = make_double2(0.0, 0.0);
    if (tid == 0) status[b] = 0;
    return;
  }
  auto at = [](int r, int c) { return r * (r + 1) / 2 + c; };
  const double2* Rb = R + b * M * M;
  for (int e = tid; e < M * M; e += kThreads) {
    const int r = e / M, c = e - r * M;
    if (c <= r) {
      double2 v = Rb[e];
      if (c == r) v.y = 0.0;
      L[at(r, c)] = v;
    }
  }
  for (int e = tid; e < MD; e += kThreads) Z[e] = P[b * MD + e];
  int st = 0;
  for (int j = 0; j < M; ++j) {
    __syncthreads();
    const double piv = L[at(j, j)].x;
    if (!(piv > 0.0) || !isfinite(piv)) {  // the same value in every thread
      st = (int)PBBSS_ST_NOT_POSDEF;
      break;
    }
    const double dj = sqrt(piv), inv = 1.0 / dj;
    for (int r = j + 1 + tid; r < M; r += kThreads) {
      double2 v = L[at(r, j)];
      L[at(r, j)] = make_double2(v.x * inv, v.y * inv);
    }
    __syncthreads();  // the pivot has been read, column j is scaled
    if (tid == 0) {
      L[at(j, j)] = make_double2(dj, 0.0);
      invd[j] = inv;
    }
    // a_rc -= l_rj conj(l_cj) on a 16 x 16 grid of threads: rows by tid / 16, columns by tid % 16
    for (int r = j + 1 + (tid >> 4); r < M; r += kThreads / 16) {
      const double2 lr = L[at(r, j)];
      for (int c = j + 1 + (tid & 15); c <= r; c += 16) {
        const double2 lc = L[at(c, j)];
        double2 v = L[at(r, c)];
        v.x -= lr.x * lc.x + lr.y * lc.y;
        v.y -= lr.y * lc.x - lr.x * lc.y;
        L[at(r, c)] = v;
      }
    }
  }
  if (st) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int e = tid; e < MD; e += kThreads) Gb[e] = make_double2(nan, nan);
    if (tid == 0) status[b] = st;
    return;
  }
  // L W = P: row j is final when step j begins; W_j = Z_j / l_jj is formed on the fly
  for (int j = 0; j < M - 1; ++j) {
    __syncthreads();
    const double inv = invd[j];
    const int d = tid & 15;  // D <= 16 columns by tid % 16, rows by tid / 16
    if (d < D) {
      const double2 zj = Z[j * D + d];
      const double wr = zj.x * inv, wi = zj.y * inv;
      for (int r = j + 1 + (tid >> 4); r < M; r += kThreads / 16) {
        const double2 l = L[at(r, j)];
        double2 v = Z[r * D + d];
        v.x -= l.x * wr - l.y * wi;
        v.y -= l.x * wi + l.y * wr;
        Z[r * D + d] = v;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < MD; e += kThreads) {
    const double inv = invd[e / D];
    Z[e] = make_double2(Z[e].x * inv, Z[e].y * inv);
  }
  // L^H G = W, from the last row up
  for (int j = M - 1; j > 0; --j) {
    __syncthreads();
    const double inv = invd[j];
    const int d = tid & 15;
    if (d < D) {
      const double2 zj = Z[j * D + d];
      const double gr = zj.x * inv, gi = zj.y * inv;
      for (int r = tid >> 4; r < j; r += kThreads / 16) {
        const double2 l = L[at(j, r)];  // conj(l_jr) g_j
        double2 v = Z[r * D + d];
        v.x -= l.x * gr + l.y * gi;
        v.y -= l.x * gi - l.y * gr;
        Z[r * D + d] = v;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < MD; e += kThreads) {
    const double inv = invd[e / D];
    Gb[e] = make_double2(Z[e].x * inv, Z[e].y * inv);
  }
  if (tid == 0) status[b] = 0;
}

// ---------------------------------------------------------------------------------------- apply
// LDS: G [M][D] | past [D][(kWpeApplyFrames + taps - 1) | 1] complex128
template <int DP>
__global__ __launch_bounds__(kThreads) void wpe_apply_kernel(WpeFrames y, const double2* G,
                                                             int taps, int delay, int tiles,
                                                             void* out_x, double* out_power) {
  extern __shared__ double2 wpe_lds[];
  static_assert(kWpeApplyFrames == kThreads, "one thread per frame");
  static_assert(kWpeMaxD <= 16, "the solver spreads the columns of P over tid % 16");
  const int tid = threadIdx.x;
  const int D = y.D, M = D * taps, WP = (kWpeApplyFrames + taps - 1) | 1;
  const int64_t b = blockIdx.x / tiles;
  const int64_t t0 = (int64_t)(blockIdx.x - b * tiles) * kWpeApplyFrames;
  double2* Gs = wpe_lds;
  double2* past = Gs + M * D;
  for (int e = tid; e < M * D; e += kThreads) Gs[e] = G[b * M * D + e];
  stage_rows(y, b, t0 - delay - taps + 1, kWpeApplyFrames + taps - 1, WP, past, tid);
  __syncthreads();
  const int64_t t = t0 + tid;
  if (t >= y.T) return;
  double ar[DP], ai[DP];
#pragma unroll
  for (int d = 0; d < DP; ++d) {
    ar[d] = ai[d] = 0.0;
    if (d < D) {
      const double2 v = load_frame(y, b * y.sb + d * y.sd + t * y.st);
      ar[d] = v.x;
      ai[d] = v.y;
    }
  }
  for (int k = 0; k < taps; ++k)
    for (int dd = 0; dd < D; ++dd) {
      const double2 v = past[dd * WP + tid + taps - 1 - k];
      const double2* g = Gs + (k * D + dd) * D;
#pragma unroll
      for (int d = 0; d < DP; ++d)
        if (d < D) {  // - conj(g_md) ytilde_m
          const double2 gv = g[d];
          ar[d] -= gv.x * v.x + gv.y * v.y;
          ai[d] -= gv.x * v.y - gv.y * v.x;
        }
    }
  double pw = 0.0;
#pragma unroll
  for (int d = 0; d < DP; ++d)
    if (d < D) {
      pw += ar[d] * ar[d] + ai[d] * ai[d];
      if (out_x) {
        const int64_t i = b * y.sb + d * y.sd + t * y.st;
        if (y.c128)
          static_cast<double2*>(out_x)[i] = make_double2(ar[d], ai[d]);
        else
          static_cast<float2*>(out_x)[i] = make_float2((float)ar[d], (float)ai[d]);
      }
    }
  if (out_power) out_power[b * y.T + t] = pw / (double)D;
}

inline int hip_ok() { return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP; }

}  // namespace

int launch_wpe_inverse_power(const WpeFrames& y, const double* raw, int64_t B, int64_t psd_context,
                             double* raw_work, double* out_power, double* out_inv, double* out_pmax,
                             hipStream_t s) {
  if (!raw) {
    const int64_t tiles = (y.T + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(wpe_power_kernel, dim3((unsigned)(B * tiles)), dim3(kThreads), 0, s, y,
                       (int)tiles, raw_work);
    raw = raw_work;
  }
  hipLaunchKernelGGL(wpe_weight_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, raw, y.T,
                     psd_context, out_power, out_inv, out_pmax);
  return hip_ok();
}

int launch_wpe_correlations(const WpeFrames& y, int64_t B, const double* inv, int taps, int delay,
                            int valid, double* part, double* out_R, double* out_P, hipStream_t s) {
  const int tiles = wpe_tiles(y.D, taps);
  const int64_t spans = wpe_spans(y.T);
  const size_t lds = wpe_corr_lds(y.D, taps);
  const int per_wave = (tiles + 3) / 4;
  double2* p2 = reinterpret_cast<double2*>(part);
  auto run = [&](auto tpw) {
    auto* kfn = wpe_corr_kernel<decltype(tpw)::value>;
    if (!raise_lds_attribute(kfn, lds)) return (int)PBBSS_ERR_LDS_CAPACITY;
    hipLaunchKernelGGL(kfn, dim3((unsigned)(B * spans)), dim3(kThreads), lds, s, y, inv, taps,
                       delay, valid, (int)spans, tiles, p2);
    return (int)PBBSS_OK;
  };
  constexpr int T0 = kWpeCorrTiles[0], T1 = kWpeCorrTiles[1], T2 = kWpeCorrTiles[2];
  const int rc = dispatch_list<T0, T1, T2>(per_wave <= T0 ? T0 : per_wave <= T1 ? T1 : T2, run);
  if (rc != PBBSS_OK) return rc;
  const int64_t total = B * tiles * 256;
  hipLaunchKernelGGL(wpe_corr_finish_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, p2, total, y.D, taps, (int)spans, tiles,
                     reinterpret_cast<double2*>(out_R), reinterpret_cast<double2*>(out_P));
  return hip_ok();
}

int launch_wpe_solve(const double* R, const double* P, const double* pmax, int64_t B, int D,
                     int taps, double* out_G, int32_t* out_status, hipStream_t s) {
  const size_t lds = wpe_solve_lds(D, taps);
  auto* kfn = wpe_solve_kernel;
  if (!raise_lds_attribute(kfn, lds)) return PBBSS_ERR_LDS_CAPACITY;
  hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(kThreads), lds, s,
                     reinterpret_cast<const double2*>(R), reinterpret_cast<const double2*>(P), pmax,
                     D, taps, reinterpret_cast<double2*>(out_G), out_status);
  return hip_ok();
}

int launch_wpe_apply(const WpeFrames& y, int64_t B, const double* G, int taps, int delay,
                     void* out_x, double* out_power, hipStream_t s) {
  const size_t lds = wpe_apply_lds(y.D, taps);
  const int64_t tiles = (y.T + kWpeApplyFrames - 1) / kWpeApplyFrames;
  auto run = [&](auto dp) {
    auto* kfn = wpe_apply_kernel<decltype(dp)::value>;
    if (!raise_lds_attribute(kfn, lds)) return (int)PBBSS_ERR_LDS_CAPACITY;
    hipLaunchKernelGGL(kfn, dim3((unsigned)(B * tiles)), dim3(kThreads), lds, s, y,
                       reinterpret_cast<const double2*>(G), taps, delay, (int)tiles, out_x,
                       out_power);
    return hip_ok();
  };
  constexpr int D0 = kWpeApplyD[0], D1 = kWpeApplyD[1], D2 = kWpeApplyD[2];
  static_assert(D2 == kWpeMaxD);
  return dispatch_list<D0, D1, D2>(y.D <= D0 ? D0 : y.D <= D1 ? D1 : D2, run);
}

}  // namespace pbbss
