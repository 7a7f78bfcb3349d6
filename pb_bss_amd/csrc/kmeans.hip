// k-means on real embeddings (reference: pb_bss/distribution/gmm.py:176-230, which hands the
// work to sklearn's KMeans; restated here from the published algorithm: Lloyd's iteration with
// sklearn's stopping rule and empty-cluster relocation, and greedy k-means++ seeding).
//
// Lloyd sweep: ONE pass over the caller's row-major (N, E) rows per iteration, the idiom of
// vmf_em_kernel (embed.hip).  A workgroup owns a chunk of L rows and walks it in tiles of R rows
// staged in LDS (16-byte loads where the rows allow it; LDS row stride E | 1).  From the staged
// tile:
//   label part  thread = row: the K squared distances as the direct sum of (x_e - c_e)^2 in
//               float64 on the exactly widened values, argmin with the lowest index winning a
//               tie, the minimum, whether the label moved;
//   sum part    thread = (row slot, column): the row is added to the sum of its class -- in
//               registers for K <= 8, E <= 64, in LDS beyond.
// Every workgroup writes its partials (class sums, counts, inertia, moved labels) to its own place;
// kmeans_finalize_kernel adds them in chunk order.  No float atomics anywhere: the order of every
// floating-point sum is fixed by the shape alone, so two calls give the same bits.
//
// The data-dependent stop lives on the device: finalize sets the problem's state, and the sweeps
// and finalizes that the host has already enqueued behind it return at once.
#include "kmeans.hpp"
#include "launch_util.hpp"

#include <algorithm>

namespace pbbss {
namespace {

constexpr int kT = kKmeansThreads;

inline int hip_ok() { return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP; }

// sum of one value per thread, in a fixed tree order; sm holds kT doubles
__device__ inline double block_sum(double v, double* sm) {
  const int tid = threadIdx.x;
  sm[tid] = v;
  __syncthreads();
  for (int o = kT / 2; o > 0; o >>= 1) {
    if (tid < o) sm[tid] += sm[tid + o];
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();
  return r;
}

__device__ inline double load_y(const void* y, int is_f64, size_t i) {
  return is_f64 ? static_cast<const double*>(y)[i] : (double)static_cast<const float*>(y)[i];
}

// ------------------------------------------------------------------------------- Lloyd sweep
struct SweepArgs {
  const void* y;
  const double* cen;     // (B, K, E)
  const uint8_t* sal;    // (B, N) or null
  int32_t* labels;       // (B, N)
  double* mind;          // (B, N), Lloyd mode only
  double* part;          // (B, C, P)
  const int32_t* state;  // (B)
  void* onehot;          // (B, K, N) in the dtype of y or null, final mode only
  int64_t N, C, L;
  int E, K, R, S, final_mode, vec;
};

template <int KT, typename TS>
__global__ void __launch_bounds__(kT) kmeans_sweep_kernel(SweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smraw[];
  constexpr int KB = KT > 0 ? KT : 8;  // classes whose distances a row keeps in registers at once
  const int E = a.E, K = a.K, R = a.R, S = a.S, ES = E | 1;
  const int KA = KT > 0 ? KT : K;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / a.C;
  const int64_t c = blockIdx.x - b * a.C;
  const int64_t N = a.N;
  const int st = a.state[b];
  if (!a.final_mode && st != kKmeansRunning) return;
  double* red = reinterpret_cast<double*>(smraw);     // [S][KA][E]
  double* dred = red + (size_t)S * KA * E;            // [kT]
  TS* tile = reinterpret_cast<TS*>(dred + kT);        // [R][ES]
  int* labs = reinterpret_cast<int*>(tile + (size_t)R * ES);  // [R] class of a selected row, -1
  int* cnt = labs + R;                                // [K]
  int* chg = cnt + K;                                 // [1]
  const bool sums = !a.final_mode;
  if (tid < K) cnt[tid] = 0;
  if (tid == 0) chg[0] = 0;
  if (KT == 0 && sums)
    for (int i = tid; i < S * KA * E; i += kT) red[i] = 0.0;
  const int s = tid / E, d = tid - s * E;
  const bool active = s < S;
  double acc[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) acc[k] = 0.0;
  double inertia = 0.0;
  const double* cen = a.cen + (size_t)b * K * E;
  const TS* y = static_cast<const TS*>(a.y);
  constexpr int VW = 16 / (int)sizeof(TS);
  typedef TS VecT __attribute__((ext_vector_type(VW)));
  const int64_t n0 = c * a.L;
  const int64_t n1 = (n0 + a.L < N) ? (n0 + a.L) : N;
  for (int64_t nb = n0; nb < n1; nb += R) {
    const int rows = (int)((n1 - nb < R) ? (n1 - nb) : R);
    const int total = rows * E;
    const TS* base = y + ((size_t)b * N + nb) * E;
    __syncthreads();  // previous tile consumed (first round: the zeroing above)
    constexpr int U = 4;
    if (a.vec) {  // E a multiple of the vector: a vector never crosses a row
      const int nv = total / VW;
      const VecT* vbase = reinterpret_cast<const VecT*>(base);
      for (int i0 = tid; i0 < nv; i0 += U * kT) {
        VecT raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * kT;
          raw[u] = vbase[i < nv ? i : nv - 1];  // clamped, masked at the LDS store
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * kT;
          if (i < nv) {
            const int e0 = i * VW;
            const int r = e0 / E;
            TS* dst = tile + (size_t)r * ES + (e0 - r * E);
#pragma unroll
            for (int x = 0; x < VW; ++x) dst[x] = raw[u][x];
          }
        }
      }
    } else {
      for (int i0 = tid; i0 < total; i0 += U * kT) {
        TS raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * kT;
          raw[u] = base[i < total ? i : total - 1];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * kT;
          if (i < total) {
            const int r = i / E;
            tile[(size_t)r * ES + (i - r * E)] = raw[u];
          }
        }
      }
    }
    __syncthreads();
    // ---- label part: thread = row
    if (tid < rows) {
      const TS* row = tile + (size_t)tid * ES;
      const int64_t n = nb + tid;
      const size_t gi = (size_t)b * N + n;
      const int old = (a.final_mode && st != kKmeansStrict) ? -1 : a.labels[gi];
      double best = 0.0, own = 0.0;
      int bk = 0;
      for (int k0 = 0; k0 < K; k0 += KB) {
        double dist[KB];
        const double* ck[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          dist[j] = 0.0;
          ck[j] = cen + (size_t)(k0 + j < K ? k0 + j : K - 1) * E;  // clamped, masked below
        }
        for (int e = 0; e < E; ++e) {
          const double v = (double)row[e];
#pragma unroll
          for (int j = 0; j < KB; ++j) {
            const double df = v - ck[j][e];
            dist[j] = fma(df, df, dist[j]);
          }
        }
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          const int k = k0 + j;
          if (k < K) {
            if (k == 0 || dist[j] < best) {  // strict: the lowest index wins a tie
              best = dist[j];
              bk = k;
            }
            if (k == old) own = dist[j];
          }
        }
      }
      const bool sel = a.sal ? a.sal[gi] != 0 : true;
      int lab = bk;
      double dmin = best;
      if (a.final_mode && st == kKmeansStrict && old >= 0 && old < K) {
        lab = old;
        dmin = own;
      }
      a.labels[gi] = lab;
      if (sel) inertia += dmin;
      if (!a.final_mode) {
        a.mind[gi] = dmin;
        if (sel) {
          atomicAdd(&cnt[lab], 1);  // integer: exact in any order
          if (lab != old) atomicAdd(&chg[0], 1);
        }
        labs[tid] = sel ? lab : -1;
      } else if (a.onehot) {
        TS* oh = static_cast<TS*>(a.onehot) + (size_t)b * K * N + n;
        for (int k = 0; k < K; ++k) oh[(size_t)k * N] = (k == lab) ? (TS)1 : (TS)0;
      }
    }
    if (!sums) continue;
    __syncthreads();
    // ---- sum part: thread = (row slot, column)
    if (active) {
      for (int r = s; r < rows; r += S) {
        const int lab = labs[r];
        const double v = (double)tile[(size_t)r * ES + d];
        if (KT > 0) {
#pragma unroll
          for (int k = 0; k < KB; ++k) acc[k] += (lab == k) ? v : 0.0;
        } else if (lab >= 0) {
          red[((size_t)s * KA + lab) * E + d] += v;  // this thread's own column of slot s
        }
      }
    }
  }
  const size_t P = (size_t)K * (E + 1) + 2;
  double* dst = a.part + ((size_t)b * a.C + c) * P;
  const double itot = block_sum(inertia, dred);
  if (tid == 0) dst[P - 2] = itot;
  if (!sums) return;
  if (KT > 0 && active) {
#pragma unroll
    for (int k = 0; k < KB; ++k) red[((size_t)s * KA + k) * E + d] = acc[k];
  }
  __syncthreads();
  for (int i = tid; i < K * E; i += kT) {
    const int k = i / E, dd = i - k * E;
    double t = 0.0;
    for (int ss = 0; ss < S; ++ss) t += red[((size_t)ss * KA + k) * E + dd];
    dst[(size_t)k * (E + 1) + dd] = t;
  }
  if (tid < K) dst[(size_t)tid * (E + 1) + E] = (double)cnt[tid];
  if (tid == 0) dst[P - 1] = (double)chg[0];
}

// ------------------------------------------------------------------------------- finalize
struct FinArgs {
  const void* y;
  const uint8_t* sal;
  const int32_t* labels;
  const double* mind;
  const double* part;
  double* tot;
  double* cen;
  const double* tol_abs;
  int32_t* state;
  int32_t* n_iter;
  int32_t* flags;
  int64_t N, C;
  int E, K, is_f64, it, max_iter;
};

// One workgroup per problem: partials in chunk order, empty classes moved onto the rows farthest
// from their centres, new centres, total squared shift, the stopping rule.
__global__ void __launch_bounds__(kT) kmeans_finalize_kernel(FinArgs a) {
  __shared__ double sd[kT];
  __shared__ int si[kT];
  __shared__ double cntd[kKmeansMaxK];
  __shared__ int empty[kKmeansMaxK];
  __shared__ int n_empty_s, far_s;
  __shared__ double fard_s, changed_s;
  const int64_t b = blockIdx.x;
  if (a.state[b] != kKmeansRunning) return;
  const int tid = threadIdx.x;
  const int E = a.E, K = a.K;
  const int64_t N = a.N;
  const size_t W = (size_t)K * (E + 1), P = W + 2;
  double* tot = a.tot + (size_t)b * W;
  for (size_t i = tid; i < P; i += kT) {
    const double* src = a.part + (size_t)b * a.C * P + i;
    double t = 0.0;
#pragma unroll 8
    for (int64_t c = 0; c < a.C; ++c) t += src[(size_t)c * P];
    if (i < W) {
      tot[i] = t;
      const size_t k = i / (E + 1);
      if (i - k * (E + 1) == (size_t)E) cntd[k] = t;
    } else if (i == P - 1) {
      changed_s = t;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int ne = 0;
    for (int k = 0; k < K; ++k)
      if (cntd[k] == 0.0) empty[ne++] = k;
    n_empty_s = ne;
  }
  __syncthreads();
  const int n_empty = n_empty_s;
  double prevd = __builtin_inf();
  int64_t prevn = -1;
  for (int j = 0; j < n_empty; ++j) {
    // the farthest selected row after (prevd, prevn) in the order: distance down, index up
    double bd = -1.0;
    int bn = -1;
    for (int64_t n = tid; n < N; n += kT) {
      const size_t gi = (size_t)b * N + n;
      if (a.sal && a.sal[gi] == 0) continue;
      const double dv = a.mind[gi];
      const bool after = dv < prevd || (dv == prevd && n > prevn);
      if (after && dv > bd) {
        bd = dv;
        bn = (int)n;
      }
    }
    sd[tid] = bd;
    si[tid] = bn;
    __syncthreads();
    if (tid == 0) {
      double fd = -1.0;
      int fn = -1;
      for (int i = 0; i < kT; ++i)
        if (si[i] >= 0 && (sd[i] > fd || (sd[i] == fd && si[i] < fn))) {
          fd = sd[i];
          fn = si[i];
        }
      far_s = fn;
      fard_s = fd;
    }
    __syncthreads();
    const int fn = far_s;
    if (fn < 0) break;  // uniform: no selected row left
    const int old = a.labels[(size_t)b * N + fn];
    const int nw = empty[j];
    if (old >= 0 && old < K) {
      for (int e = tid; e < E; e += kT) {
        const double x = load_y(a.y, a.is_f64, ((size_t)b * N + fn) * E + e);
        tot[(size_t)old * (E + 1) + e] -= x;
        tot[(size_t)nw * (E + 1) + e] = x;
      }
      if (tid == 0) {
        cntd[nw] = 1.0;
        cntd[old] -= 1.0;
      }
    }
    prevd = fard_s;
    prevn = fn;
    __syncthreads();
  }
  double sh = 0.0;
  double* cen = a.cen + (size_t)b * K * E;
  for (int i = tid; i < K * E; i += kT) {
    const int k = i / E, e = i - k * E;
    const double cn = cntd[k];
    const double old = cen[i];
    const double nw = cn > 0.0 ? tot[(size_t)k * (E + 1) + e] / cn : old;  // empty: stays
    const double df = nw - old;
    sh = fma(df, df, sh);
    cen[i] = nw;
  }
  const double shift = block_sum(sh, sd);
  if (tid == 0) {
    a.n_iter[b] = a.it + 1;
    int ns = kKmeansRunning;
    if (changed_s == 0.0)
      ns = kKmeansStrict;
    else if (shift <= a.tol_abs[b])
      ns = kKmeansRelabel;
    else if (a.it + 1 >= a.max_iter)
      ns = kKmeansRelabel;
    if (ns != kKmeansRunning) {
      a.state[b] = ns;
      atomicSub(&a.flags[0], 1);
    }
  }
}

// inertia of the last sweep: chunk partials in order
__global__ void __launch_bounds__(kT)
    kmeans_inertia_kernel(const double* part, int64_t B, int64_t C, size_t P, double* inertia) {
  const int64_t b = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (b >= B) return;
  double t = 0.0;
  for (int64_t c = 0; c < C; ++c) t += part[((size_t)b * C + c) * P + P - 2];
  inertia[b] = t;
}

__global__ void kmeans_flags_kernel(int32_t* flags, int running) {
  flags[0] = running;
  flags[1] = 0;
}

// ------------------------------------------------------------------------------- tolerance
// tol * mean_e var_n x over the selected rows: column sums, then squared deviations from the
// finished column means (two passes, as numpy.var).  part (B, C, E + 1): columns | selected rows.
template <typename TS>
__global__ void __launch_bounds__(kT)
    kmeans_moment_kernel(const TS* y, const uint8_t* sal, const double* mean, double* part,
                         int64_t N, int64_t C, int64_t L, int E) {
  __shared__ double sm[kT];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / C;
  const int64_t c = blockIdx.x - b * C;
  const int S = kT / E;
  const int s = tid / E, d = tid - s * E;
  const int64_t n0 = c * L;
  const int64_t n1 = (n0 + L < N) ? (n0 + L) : N;
  double acc = 0.0, cnt = 0.0;
  if (s < S) {
    const double m = mean ? mean[(size_t)b * (E + 1) + d] : 0.0;
    for (int64_t n = n0 + s; n < n1; n += S) {
      const size_t gi = (size_t)b * N + n;
      if (sal && sal[gi] == 0) continue;
      const double v = (double)y[gi * E + d];
      if (mean) {
        const double df = v - m;
        acc = fma(df, df, acc);
      } else {
        acc += v;
      }
      cnt += 1.0;
    }
  }
  double* dst = part + ((size_t)b * C + c) * (E + 1);
  sm[tid] = acc;
  __syncthreads();
  if (tid < E) {
    double t = 0.0;
    for (int ss = 0; ss < S; ++ss) t += sm[ss * E + tid];
    dst[tid] = t;
  }
  __syncthreads();
  sm[tid] = (s < S && d == 0) ? cnt : 0.0;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int ss = 0; ss < S; ++ss) t += sm[ss * E];
    dst[E] = t;
  }
}

__global__ void __launch_bounds__(kT)
    kmeans_moment_finish_kernel(const double* part, double* mean, double* tol_abs, int32_t* state,
                                int32_t* flags, int64_t C, int E, int K, int pass, double tol) {
  __shared__ double sm[kKmeansMaxE + 1];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  for (int i = tid; i <= E; i += kT) {
    double t = 0.0;
    for (int64_t c = 0; c < C; ++c) t += part[((size_t)b * C + c) * (E + 1) + i];
    sm[i] = t;
  }
  __syncthreads();
  const double n_sel = sm[E];
  if (pass == 0) {
    for (int i = tid; i < E; i += kT) mean[(size_t)b * (E + 1) + i] = n_sel > 0 ? sm[i] / n_sel : 0.0;
    if (tid == 0) {
      mean[(size_t)b * (E + 1) + E] = n_sel;
      if (n_sel < (double)K) {  // as sklearn: n_samples should be >= n_clusters
        state[b] = kKmeansInvalid;
        atomicSub(&flags[0], 1);
        atomicExch(&flags[1], 1);
      }
    }
  } else if (tid == 0) {
    double t = 0.0;
    for (int e = 0; e < E; ++e) t += n_sel > 0 ? sm[e] / n_sel : 0.0;
    tol_abs[b] = tol * (t / E);
  }
}

// ------------------------------------------------------------------------------- k-means++
// closest_dist_sq of every row against the centre just chosen and the chunk sums of
// v_n = selected(n) * closest_n that the prefix search walks.  Without a centre (before the first
// draw) v_n = selected(n): the uniform draw goes through the same search.
template <typename TS>
__global__ void __launch_bounds__(kT)
    kpp_update_kernel(const TS* y, const uint8_t* sal, const int32_t* chosen, int first,
                      double* closest, double* csum, int64_t N, int64_t nch, int E) {
  __shared__ double sm[kT];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / nch;
  const int64_t c = blockIdx.x - b * nch;
  const TS* cr = chosen ? y + ((size_t)b * N + chosen[b]) * E : nullptr;
  double t = 0.0;
  for (int u = 0; u < kKmeansScanRows / kT; ++u) {
    const int64_t n = c * kKmeansScanRows + (int64_t)u * kT + tid;  // coalesced over the lanes
    if (n >= N) break;
    const size_t gi = (size_t)b * N + n;
    const bool sel = sal ? sal[gi] != 0 : true;
    double v = 1.0;
    if (cr) {
      const TS* row = y + gi * E;
      double dd = 0.0;
      for (int e = 0; e < E; ++e) {
        const double df = (double)row[e] - (double)cr[e];
        dd = fma(df, df, dd);
      }
      v = first ? dd : fmin(closest[gi], dd);
      closest[gi] = v;
    }
    t += sel ? v : 0.0;
  }
  const double r = block_sum(t, sm);
  if (tid == 0) csum[(size_t)b * nch + c] = r;
}

// One workgroup per problem: the ordered prefix sum of v -- a scan of the chunk sums, then a scan
// within the chunk a target falls into -- searched for `trials` targets rnd_j * potential.
// right = 0: first row whose prefix reaches the target (searchsorted side='left');
// right = 1: first row whose prefix exceeds it (side='right': the uniform first draw).
__global__ void __launch_bounds__(kT)
    kpp_search_kernel(const uint8_t* sal, const double* closest, const double* csum,
                      const double* rnd, int64_t rnd_stride, int rnd_off, int trials, int right,
                      int32_t* cand, int64_t N, int64_t nch) {
  __shared__ double seg[kT];
  __shared__ double segoff[kT + 1];
  __shared__ double target[kKmeansMaxTrials], cbase[kKmeansMaxTrials];
  __shared__ long long cchunk[kKmeansMaxTrials];
  __shared__ int hit_s, last_s;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double* cs = csum + (size_t)b * nch;
  const int64_t per = (nch + kT - 1) / kT;
  const int64_t c0 = tid * per < nch ? tid * per : nch;
  const int64_t c1 = c0 + per < nch ? c0 + per : nch;
  {
    double t = 0.0;
    for (int64_t c = c0; c < c1; ++c) t += cs[c];
    seg[tid] = t;
  }
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    for (int i = 0; i < kT; ++i) {
      segoff[i] = run;
      run += seg[i];
    }
    segoff[kT] = run;
  }
  __syncthreads();
  const double pot = segoff[kT];
  if (tid < trials) {
    target[tid] = rnd[(size_t)b * rnd_stride + rnd_off + tid] * pot;
    cchunk[tid] = -1;
  }
  __syncthreads();
  {
    // the intervals [run, next) of this thread's chunks tile [segoff[tid], segoff[tid + 1]) exactly
    double run = segoff[tid];
    const double end = segoff[tid + 1];
    for (int64_t c = c0; c < c1; ++c) {
      const double next = (c == c1 - 1) ? end : fmin(run + cs[c], end);
      for (int j = 0; j < trials; ++j) {
        const double tg = target[j];
        const bool hit = right ? (run <= tg && tg < next) : (run < tg && tg <= next);
        if (hit) {
          cchunk[j] = c;
          cbase[j] = run;
        }
      }
      run = next;
    }
  }
  __syncthreads();
  constexpr int RPT = kKmeansScanRows / kT;
  for (int j = 0; j < trials; ++j) {
    const long long c = cchunk[j];
    const double tg = target[j];
    if (c < 0) {  // target outside the prefix range: numpy's searchsorted ends, clipped
      if (tid == 0) cand[b * kKmeansMaxTrials + j] = (!right && tg <= 0.0) ? 0 : (int32_t)(N - 1);
      continue;
    }
    if (tid == 0) {
      hit_s = 0x7fffffff;
      last_s = 0;
    }
    double v[RPT];
    double t = 0.0;
    for (int u = 0; u < RPT; ++u) {
      const int64_t n = c * kKmeansScanRows + (int64_t)tid * RPT + u;
      v[u] = 0.0;
      if (n < N) {
        const size_t gi = (size_t)b * N + n;
        const bool sel = sal ? sal[gi] != 0 : true;
        if (sel) v[u] = closest ? closest[gi] : 1.0;
      }
      t += v[u];
    }
    seg[tid] = t;
    __syncthreads();
    if (tid == 0) {
      double run = cbase[j];
      for (int i = 0; i < kT; ++i) {
        segoff[i] = run;
        run += seg[i];
      }
      segoff[kT] = run;
    }
    __syncthreads();
    double run = segoff[tid];
    const double end = segoff[tid + 1];
    for (int u = 0; u < RPT; ++u) {
      const int loc = tid * RPT + u;
      const double next = (u == RPT - 1) ? end : fmin(run + v[u], end);
      const bool hit = right ? (run <= tg && tg < next) : (run < tg && tg <= next);
      if (hit) atomicMin(&hit_s, loc);
      if (v[u] > 0.0) atomicMax(&last_s, loc);
      run = next;
    }
    __syncthreads();
    if (tid == 0) {
      // beyond the chunk's own scan by a rounding: its last row of positive weight
      const int loc = hit_s != 0x7fffffff ? hit_s : last_s;
      int64_t n = c * kKmeansScanRows + loc;
      if (n > N - 1) n = N - 1;
      cand[b * kKmeansMaxTrials + j] = (int32_t)n;
    }
    __syncthreads();
  }
}

// potentials of all candidates in one pass: cpart (B, nch, kKmeansMaxTrials)
template <typename TS>
__global__ void __launch_bounds__(kT)
    kpp_candidates_kernel(const TS* y, const uint8_t* sal, const double* closest,
                          const int32_t* cand, int trials, double* cpart, int64_t N, int64_t nch,
                          int E) {
  __shared__ double sm[kT];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / nch;
  const int64_t c = blockIdx.x - b * nch;
  const TS* cr[kKmeansMaxTrials];
#pragma unroll
  for (int j = 0; j < kKmeansMaxTrials; ++j)
    cr[j] = y + ((size_t)b * N + cand[b * kKmeansMaxTrials + (j < trials ? j : 0)]) * E;
  double pot[kKmeansMaxTrials];
#pragma unroll
  for (int j = 0; j < kKmeansMaxTrials; ++j) pot[j] = 0.0;
  for (int u = 0; u < kKmeansScanRows / kT; ++u) {
    const int64_t n = c * kKmeansScanRows + (int64_t)u * kT + tid;  // coalesced over the lanes
    if (n >= N) break;
    const size_t gi = (size_t)b * N + n;
    if (sal && sal[gi] == 0) continue;
    const TS* row = y + gi * E;
    double dd[kKmeansMaxTrials];
#pragma unroll
    for (int j = 0; j < kKmeansMaxTrials; ++j) dd[j] = 0.0;
    for (int e = 0; e < E; ++e) {
      const double v = (double)row[e];
#pragma unroll
      for (int j = 0; j < kKmeansMaxTrials; ++j) {
        const double df = v - (double)cr[j][e];
        dd[j] = fma(df, df, dd[j]);
      }
    }
    const double cl = closest[gi];
#pragma unroll
    for (int j = 0; j < kKmeansMaxTrials; ++j) pot[j] += fmin(cl, dd[j]);
  }
  double* dst = cpart + ((size_t)b * nch + c) * kKmeansMaxTrials;
#pragma unroll
  for (int j = 0; j < kKmeansMaxTrials; ++j) {
    const double r = block_sum(pot[j], sm);
    if (tid == 0) dst[j] = r;
  }
}

// One workgroup per problem: candidate potentials in chunk order, the first minimum wins; the
// chosen row becomes centre `step`.
__global__ void __launch_bounds__(kT)
    kpp_pick_kernel(const void* y, int is_f64, const double* cpart, const int32_t* cand,
                    int trials, int step, int32_t* chosen, int32_t* indices, double* centers,
                    int64_t N, int64_t nch, int E, int K) {
  __shared__ double pot[kKmeansMaxTrials];
  __shared__ int pick_s;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (cpart && tid < trials) {
    double t = 0.0;
    for (int64_t c = 0; c < nch; ++c) t += cpart[((size_t)b * nch + c) * kKmeansMaxTrials + tid];
    pot[tid] = t;
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    if (cpart)
      for (int j = 1; j < trials; ++j)
        if (pot[j] < pot[best]) best = j;
    const int32_t n = cand[b * kKmeansMaxTrials + best];
    pick_s = n;
    chosen[b] = n;
    indices[b * K + step] = n;
  }
  __syncthreads();
  const int64_t n = pick_s;
  for (int e = tid; e < E; e += kT)
    centers[((size_t)b * K + step) * E + e] = load_y(y, is_f64, ((size_t)b * N + n) * E + e);
}

// ------------------------------------------------------------------------------- launchers
template <int KT, typename TS>
int launch_sweep_kt(const KmeansGeom& g, const SweepArgs& a, hipStream_t s) {
  auto kern = kmeans_sweep_kernel<KT, TS>;
  if (g.lds > 64 * 1024 && !raise_lds_attribute(kern, g.lds)) return PBBSS_ERR_HIP;
  hipLaunchKernelGGL(kern, dim3((unsigned)(g.B * g.C)), dim3(kT), g.lds, s, a);
  return hip_ok();
}

template <typename TS>
int launch_sweep_t(const KmeansGeom& g, const SweepArgs& a, hipStream_t s) {
  switch (g.KT) {
    case 2: return launch_sweep_kt<2, TS>(g, a, s);
    case 3: return launch_sweep_kt<3, TS>(g, a, s);
    case 4: return launch_sweep_kt<4, TS>(g, a, s);
    case 8: return launch_sweep_kt<8, TS>(g, a, s);
    default: return launch_sweep_kt<0, TS>(g, a, s);
  }
}

int launch_sweep(const KmeansGeom& g, SweepArgs a, hipStream_t s) {
  a.N = g.N;
  a.C = g.C;
  a.L = g.L;
  a.E = g.E;
  a.K = g.K;
  a.R = g.R;
  a.S = g.S;
  const int vw = g.is_f64 ? 2 : 4;
  a.vec = g.E % vw == 0 && reinterpret_cast<uintptr_t>(a.y) % 16 == 0;
  return g.is_f64 ? launch_sweep_t<double>(g, a, s) : launch_sweep_t<float>(g, a, s);
}

inline unsigned blocks_for(int64_t total) { return (unsigned)((total + kT - 1) / kT); }

}  // namespace

bool kmeans_geom(int64_t B, int64_t N, int E, int K, int is_f64, KmeansGeom* g) {
  if (B < 1 || N < 1 || N > INT32_MAX || E < 1 || E > kKmeansMaxE || K < 1 || K > kKmeansMaxK)
    return false;
  g->B = B;
  g->N = N;
  g->E = E;
  g->K = K;
  g->is_f64 = is_f64;
  const bool fast = K <= kKmeansFastK && E <= kKmeansFastE;
  g->KT = !fast ? 0 : K <= 2 ? 2 : K <= 3 ? 3 : K <= 4 ? 4 : 8;
  const size_t ts = is_f64 ? 8 : 4;
  const size_t row = (size_t)(E | 1) * ts;
  const size_t tile_budget = fast ? 40 * 1024 : 16 * 1024;
  g->R = (int)std::max<size_t>(1, std::min<size_t>(kT, tile_budget / row));
  if (fast)
    g->S = kT / E;
  else
    g->S = std::max(1, std::min(kT / E, 8192 / (K * E)));
  const int KA = fast ? g->KT : K;
  g->lds = ((size_t)g->S * KA * E + kT) * sizeof(double) + (size_t)g->R * row +
           ((size_t)g->R + K + 1) * sizeof(int);
  const int64_t tiles = (N + g->R - 1) / g->R;
  int64_t C = std::max<int64_t>(1, (kKmeansTargetWorkgroups + B - 1) / B);
  C = std::min(C, tiles);
  g->L = ((tiles + C - 1) / C) * g->R;
  g->C = (N + g->L - 1) / g->L;
  g->scan_chunks = (N + kKmeansScanRows - 1) / kKmeansScanRows;
  const int64_t grid_max = (int64_t(1) << 31) - 1;
  return B <= grid_max / g->C && B <= grid_max / g->scan_chunks;
}

int run_kmeans_fit(const KmeansGeom& g, const KmeansWork& w, const void* y, const uint8_t* sal,
                   int max_iter, double tol, int block, double* centers, int32_t* labels,
                   double* inertia, int32_t* n_iter, hipStream_t s) {
  const int64_t B = g.B;
  if (hipMemsetAsync(labels, 0xff, (size_t)B * g.N * sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(w.state, 0, (size_t)B * sizeof(int32_t), s) != hipSuccess ||
      hipMemsetAsync(n_iter, 0, (size_t)B * sizeof(int32_t), s) != hipSuccess)
    return PBBSS_ERR_HIP;
  hipLaunchKernelGGL(kmeans_flags_kernel, dim3(1), dim3(1), 0, s, w.flags, (int)B);
  // tol * mean_e var_n x, once
  for (int pass = 0; pass < 2; ++pass) {
    const double* mean = pass ? w.mean : nullptr;
    const dim3 grid((unsigned)(B * g.C));
    if (g.is_f64)
      hipLaunchKernelGGL(kmeans_moment_kernel<double>, grid, dim3(kT), 0, s,
                         static_cast<const double*>(y), sal, mean, w.part, g.N, g.C, g.L, g.E);
    else
      hipLaunchKernelGGL(kmeans_moment_kernel<float>, grid, dim3(kT), 0, s,
                         static_cast<const float*>(y), sal, mean, w.part, g.N, g.C, g.L, g.E);
    hipLaunchKernelGGL(kmeans_moment_finish_kernel, dim3((unsigned)B), dim3(kT), 0, s, w.part,
                       w.mean, w.tol_abs, w.state, w.flags, g.C, g.E, g.K, pass, tol);
  }
  if (hip_ok() != PBBSS_OK) return PBBSS_ERR_HIP;
  SweepArgs sa{};
  sa.y = y;
  sa.cen = centers;
  sa.sal = sal;
  sa.labels = labels;
  sa.mind = w.mind;
  sa.part = w.part;
  sa.state = w.state;
  FinArgs fa{};
  fa.y = y;
  fa.sal = sal;
  fa.labels = labels;
  fa.mind = w.mind;
  fa.part = w.part;
  fa.tot = w.tot;
  fa.cen = centers;
  fa.tol_abs = w.tol_abs;
  fa.state = w.state;
  fa.n_iter = n_iter;
  fa.flags = w.flags;
  fa.N = g.N;
  fa.C = g.C;
  fa.E = g.E;
  fa.K = g.K;
  fa.is_f64 = g.is_f64;
  fa.max_iter = max_iter;
  int32_t flags[2] = {0, 0};
  for (int it = 0; it < max_iter;) {
    // a block of iterations; those behind the stop return at once
    const int stop = (max_iter - it < block) ? max_iter : it + block;
    for (; it < stop; ++it) {
      const int rc = launch_sweep(g, sa, s);
      if (rc != PBBSS_OK) return rc;
      fa.it = it;
      hipLaunchKernelGGL(kmeans_finalize_kernel, dim3((unsigned)B), dim3(kT), 0, s, fa);
    }
    if (hip_ok() != PBBSS_OK) return PBBSS_ERR_HIP;
    if (hipMemcpyAsync(flags, w.flags, sizeof(flags), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return PBBSS_ERR_HIP;
    if (flags[1]) return PBBSS_ERR_INVALID_ARG;
    if (flags[0] <= 0) break;
  }
  sa.final_mode = 1;
  sa.mind = nullptr;
  const int rc = launch_sweep(g, sa, s);
  if (rc != PBBSS_OK) return rc;
  hipLaunchKernelGGL(kmeans_inertia_kernel, dim3(blocks_for(B)), dim3(kT), 0, s, w.part, B, g.C,
                     kmeans_part_len(g), inertia);
  return hip_ok();
}

int run_kmeans_predict(const KmeansGeom& g, const KmeansWork& w, const void* y,
                       const double* centers, int32_t* labels, void* one_hot, double* inertia,
                       hipStream_t s) {
  if (hipMemsetAsync(w.state, 0, (size_t)g.B * sizeof(int32_t), s) != hipSuccess)
    return PBBSS_ERR_HIP;
  SweepArgs sa{};
  sa.y = y;
  sa.cen = centers;
  sa.labels = labels;
  sa.part = w.part;
  sa.state = w.state;
  sa.onehot = one_hot;
  sa.final_mode = 1;
  const int rc = launch_sweep(g, sa, s);
  if (rc != PBBSS_OK) return rc;
  if (inertia)
    hipLaunchKernelGGL(kmeans_inertia_kernel, dim3(blocks_for(g.B)), dim3(kT), 0, s, w.part, g.B,
                       g.C, kmeans_part_len(g), inertia);
  return hip_ok();
}

int run_kmeans_plusplus(const KmeansGeom& g, const KmeansSeedWork& w, const void* y,
                        const uint8_t* sal, int trials, const double* randoms, int32_t* indices,
                        double* centers, hipStream_t s) {
  const int64_t B = g.B, N = g.N, nch = g.scan_chunks;
  const int E = g.E, K = g.K;
  const int64_t rnd_stride = 1 + (int64_t)(K - 1) * trials;
  const dim3 grid((unsigned)(B * nch)), one((unsigned)B), block(kT);
  auto update = [&](const int32_t* chosen, int first) {
    if (g.is_f64)
      hipLaunchKernelGGL(kpp_update_kernel<double>, grid, block, 0, s,
                         static_cast<const double*>(y), sal, chosen, first, w.closest, w.csum, N,
                         nch, E);
    else
      hipLaunchKernelGGL(kpp_update_kernel<float>, grid, block, 0, s,
                         static_cast<const float*>(y), sal, chosen, first, w.closest, w.csum, N,
                         nch, E);
  };
  // the first centre: a uniform draw over the selected rows
  update(nullptr, 0);
  hipLaunchKernelGGL(kpp_search_kernel, one, block, 0, s, sal, (const double*)nullptr, w.csum,
                     randoms, rnd_stride, 0, 1, 1, w.cand, N, nch);
  hipLaunchKernelGGL(kpp_pick_kernel, one, block, 0, s, y, g.is_f64, (const double*)nullptr,
                     w.cand, 1, 0, w.chosen, indices, centers, N, nch, E, K);
  for (int step = 1; step < K; ++step) {
    update(w.chosen, step == 1);
    hipLaunchKernelGGL(kpp_search_kernel, one, block, 0, s, sal, (const double*)w.closest, w.csum,
                       randoms, rnd_stride, 1 + (step - 1) * trials, trials, 0, w.cand, N, nch);
    if (g.is_f64)
      hipLaunchKernelGGL(kpp_candidates_kernel<double>, grid, block, 0, s,
                         static_cast<const double*>(y), sal, (const double*)w.closest,
                         (const int32_t*)w.cand, trials, w.cpart, N, nch, E);
    else
      hipLaunchKernelGGL(kpp_candidates_kernel<float>, grid, block, 0, s,
                         static_cast<const float*>(y), sal, (const double*)w.closest,
                         (const int32_t*)w.cand, trials, w.cpart, N, nch, E);
    hipLaunchKernelGGL(kpp_pick_kernel, one, block, 0, s, y, g.is_f64, (const double*)w.cpart,
                       w.cand, trials, step, w.chosen, indices, centers, N, nch, E, K);
  }
  return hip_ok();
}

}  // namespace pbbss
