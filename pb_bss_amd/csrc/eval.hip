// Evaluation metrics on the device (include/pbbss.h, section V): si_sdr, signal power,
// input_sxr and output_sxr.
//
// All of them are streaming reductions over the N samples of time signals.  One kernel template
// serves both reads of the rows:
//   Gram pass      sum r_i^2 and sum r_i e_j of the Kr + Ke rows of a batch item, every row read
//                  once (signal power is the Kr = 1, Ke = 0 case),
//   residual pass  sum (e_j - alpha_ij r_i)^2 with alpha_ij from the finished Gram pass.
// A workgroup owns kEvalSpan samples of every row of one item: 16-byte loads where all rows of the
// item share their alignment, a scalar head and tail around them (scalar loads throughout where
// they do not), float64 accumulators in registers, a shuffle tree per wave, the four waves added in
// order, one plain store per accumulator to the workspace.  Finishing kernels add the spans in
// order.  No atomics, no waits between workgroups: the result depends on the shapes and on the
// row alignment only.  sum r_i e_j and sum r_i^2 run through the same tree in the same lanes, so an
// estimate that is c * reference with c a power of two has alpha == c exactly and a residual of
// exactly zero (the reference's doctests return inf there).
#include "eval.hpp"
#include "eval_dev.hpp"

#include <math.h>

namespace pbbss {
namespace {

template <typename T>
struct Wide;
template <>
struct Wide<float> {
  using vec = float4;
  static constexpr int V = 4;
  static __device__ void load(float (&d)[4], const float* p) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
  }
};
template <>
struct Wide<double> {
  using vec = double2;
  static constexpr int V = 2;
  static __device__ void load(double (&d)[2], const double* p) {
    const double2 v = *reinterpret_cast<const double2*>(p);
    d[0] = v.x, d[1] = v.y;
  }
};

__device__ inline unsigned low4(const void* p) {
  return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u);
}

// partials: (B, chunks, A) with A = Kr + Kr Ke (Gram: [rr_i][re_ij]) or Kr Ke (residual).
// gram: (B, Kr + Kr Ke), the finished Gram pass (residual pass only).
template <typename T, int M, bool RESID>
__global__ __launch_bounds__(kEvalThreads) void rows_kernel(EvalRows g, int64_t chunks,
                                                            const double* __restrict__ gram,
                                                            double* __restrict__ partials) {
  constexpr int V = Wide<T>::V;
  const int64_t b = (int64_t)blockIdx.x / chunks;
  const int64_t w = (int64_t)blockIdx.x - b * chunks;
  const int Kr = g.Kr, Ke = g.Ke;
  const int tid = threadIdx.x;

  const T* r[M];
  const T* e[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    r[i] = static_cast<const T*>(g.ref) + b * g.ref_batch + (i < Kr ? i : 0) * g.ref_row;
    e[i] = Ke > 0 ? static_cast<const T*>(g.est) + b * g.est_batch + (i < Ke ? i : 0) * g.est_row
                  : r[0];
  }
  const unsigned a0 = low4(r[0]);
  // the C layer refuses pointers that are no multiple of sizeof(T); never a misaligned wide load
  bool vec_ok = a0 % sizeof(T) == 0;
#pragma unroll
  for (int i = 0; i < M; ++i) vec_ok = vec_ok && low4(r[i]) == a0 && low4(e[i]) == a0;

  // samples [s0, s1) of every row: scalar [s0, first), 16-byte loads [first, tail0), scalar
  // [tail0, s1)
  const int64_t head = ((16u - a0) & 15u) / sizeof(T);
  const int64_t s0 = w * kEvalSpan;
  const int64_t s1 = g.N < s0 + kEvalSpan ? g.N : s0 + kEvalSpan;
  int64_t first = s1, nvec = 0;
  if (vec_ok) {
    const int64_t lo = s0 > head ? s0 : head;
    first = head + (lo - head + V - 1) / V * V;
    if (first > s1) first = s1;
    nvec = (s1 - first) / V;
  }
  const int64_t tail0 = first + nvec * V;

  double acc_r[M];
  double acc[M][M];
  double alpha[M][M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    acc_r[i] = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      acc[i][j] = 0.0;
      alpha[i][j] = 0.0;
    }
  }
  if (RESID) {
    const double* gb = gram + b * (int64_t)(Kr + Kr * Ke);
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j)
        if (i < Kr && j < Ke) alpha[i][j] = gb[Kr + i * Ke + j] / gb[i];
  }

  auto add = [&](const double(&rd)[M], const double(&ed)[M]) {
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if (i < Kr) {
        if (!RESID) acc_r[i] = fma(rd[i], rd[i], acc_r[i]);
#pragma unroll
        for (int j = 0; j < M; ++j) {
          if (j < Ke) {
            if (RESID) {
              const double d = fma(-alpha[i][j], rd[i], ed[j]);
              acc[i][j] = fma(d, d, acc[i][j]);
            } else {
              acc[i][j] = fma(rd[i], ed[j], acc[i][j]);
            }
          }
        }
      }
    }
  };
  auto scalar_range = [&](int64_t lo, int64_t hi) {
    for (int64_t n = lo + tid; n < hi; n += kEvalThreads) {
      double rd[M], ed[M];
#pragma unroll
      for (int i = 0; i < M; ++i) {
        rd[i] = i < Kr ? (double)r[i][n] : 0.0;
        ed[i] = i < Ke ? (double)e[i][n] : 0.0;
      }
      add(rd, ed);
    }
  };

  scalar_range(s0, first);
  for (int64_t k = tid; k < nvec; k += kEvalThreads) {
    const int64_t n = first + k * V;
    T rraw[M][V], eraw[M][V];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if (i < Kr) Wide<T>::load(rraw[i], r[i] + n);
      if (i < Ke) Wide<T>::load(eraw[i], e[i] + n);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      double rd[M], ed[M];
#pragma unroll
      for (int i = 0; i < M; ++i) {
        rd[i] = i < Kr ? (double)rraw[i][v] : 0.0;
        ed[i] = i < Ke ? (double)eraw[i][v] : 0.0;
      }
      add(rd, ed);
    }
  }
  scalar_range(tail0, s1);

  __shared__ double red[kEvalThreads / 64][M + M * M];
  const int lane = tid & 63, wv = tid >> 6;
  const int pair0 = RESID ? 0 : Kr;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    if (i < Kr) {
      if (!RESID) {
        const double s = wave_sum(acc_r[i]);
        if (lane == 0) red[wv][i] = s;
      }
#pragma unroll
      for (int j = 0; j < M; ++j) {
        if (j < Ke) {
          const double s = wave_sum(acc[i][j]);
          if (lane == 0) red[wv][pair0 + i * Ke + j] = s;
        }
      }
    }
  }
  __syncthreads();
  const int A = pair0 + Kr * Ke;
  if (tid < A) {
    double s = red[0][tid];
#pragma unroll
    for (int q = 1; q < kEvalThreads / 64; ++q) s += red[q][tid];
    partials[(int64_t)blockIdx.x * A + tid] = s;
  }
}

// out[b, a] = sum over the spans (/ divisor when it is not zero)
__global__ __launch_bounds__(256) void finish_sum_kernel(const double* __restrict__ partials,
                                                         int64_t total, int64_t chunks, int A,
                                                         double divisor, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / A;
  const int a = (int)(idx - b * A);
  const double s = span_sum(partials + b * chunks * A + a, chunks, A);
  out[idx] = divisor != 0.0 ? s / divisor : s;
}

// out[b, i, j] = 10 log10(alpha^2 rr / residual)
__global__ __launch_bounds__(256) void si_sdr_finish_kernel(const double* __restrict__ gram,
                                                            const double* __restrict__ partials,
                                                            int64_t total, int64_t chunks, int Kr,
                                                            int Ke, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int A = Kr * Ke;
  const int64_t b = idx / A;
  const int a = (int)(idx - b * A);
  const int i = a / Ke;
  const double* gb = gram + b * (int64_t)(Kr + A);
  const double rr = gb[i], re = gb[Kr + a];
  const double al = re / rr;
  const double res = span_sum(partials + b * chunks * A + a, chunks, A);
  out[idx] = 10.0 * log10(al * al * rr / res);
}

__device__ inline double sxr_db(double s, double x) { return 10.0 * log10(s / x); }

// ---- output_sxr ---------------------------------------------------------------------------
// one wave per batch item.  pS (B Ks Kt, chunks), pN (B Kt, chunks): span partials of sum |x|^2.
__global__ __launch_bounds__(64) void output_sxr_kernel(const double* __restrict__ pS,
                                                        const double* __restrict__ pN,
                                                        int64_t chunks, double count, int Ks,
                                                        int Kt, int average,
                                                        double* __restrict__ out_sxr,
                                                        int64_t* __restrict__ out_sel,
                                                        double* __restrict__ out_mean) {
  __shared__ double S[kSxrMaxTargets * kSxrMaxTargets];
  __shared__ double Nn[kSxrMaxTargets];
  __shared__ double val[3][kSxrMaxTargets];
  __shared__ int chosen[kSxrMaxTargets];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int nS = Ks * Kt;
  for (int q = lane; q < nS + Kt; q += 64) {
    if (q < nS)
      S[q] = span_sum(pS + (b * nS + q) * chunks, chunks, 1) / count;
    else
      Nn[q - nS] = span_sum(pN + (b * Kt + (q - nS)) * chunks, chunks, 1) / count;
  }
  __syncthreads();

  // radix[k]: selections that share their first k + 1 picks
  int radix[kSxrMaxTargets];
#pragma unroll
  for (int k = kSxrMaxTargets - 1; k >= 0; --k) {
    radix[k] = 1;
    if (k < Ks - 1) radix[k] = radix[k + 1 < kSxrMaxTargets ? k + 1 : k] * (Kt - 1 - k);
  }
  const int P = radix[0] * Kt;

  double best = 0.0;
  int best_p = 0x7fffffff;
  for (int p = lane; p < P; p += 64) {
    int sel[kSxrMaxTargets];
    unrank_selection(p, Ks, Kt, radix, sel);
    double v[kSxrMaxTargets];
#pragma unroll
    for (int k = 0; k < kSxrMaxTargets; ++k) v[k] = k < Ks ? S[k * Kt + sel[k]] : 0.0;
    double total;
    if (Ks == 8) {
      total = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    } else {
      total = 0.0;
#pragma unroll
      for (int k = 0; k < kSxrMaxTargets - 1; ++k)
        if (k < Ks) total += v[k];
    }
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
    unrank_selection(best_p, Ks, Kt, radix, sel);
#pragma unroll
    for (int k = 0; k < kSxrMaxTargets; ++k)
      if (k < Ks) chosen[k] = sel[k];
  }
  __syncthreads();

  if (lane < Ks) {
    const int k = lane, t = chosen[k];
    const double SS = S[k * Kt + t];
    double II = 0.0;  // the other sources in output t, in index order (Ks - 1 < 8 addends)
    for (int n = 0; n < Ks; ++n)
      if (n != k) II += S[n * Kt + t];
    const double NN = Nn[t];
    val[0][k] = sxr_db(SS, II + NN);
    val[1][k] = sxr_db(SS, II);
    val[2][k] = sxr_db(SS, NN);
    out_sel[b * Ks + k] = t;
#pragma unroll
    for (int m = 0; m < 3; ++m) out_sxr[(b * 3 + m) * Ks + k] = val[m][k];
  }
  __syncthreads();
  if (average && lane < 3) out_mean[b * 3 + lane] = np_sum(val[lane], Ks, 1) / (double)Ks;
}

// ---- input_sxr ----------------------------------------------------------------------------
// one workgroup per batch item.  pS (B K D, chunks), pN (B D, chunks).  out (B, 3, Ko, Do).
__global__ __launch_bounds__(256) void input_sxr_kernel(const double* __restrict__ pS,
                                                        const double* __restrict__ pN,
                                                        int64_t chunks, double count, int K, int D,
                                                        int avg_sources, int avg_channels,
                                                        double* __restrict__ out) {
  constexpr int KD = kSxrMaxSources * kSxrMaxSensors;
  __shared__ double S[KD], I[KD], Nn[kSxrMaxSensors];
  __shared__ double others[KD][kSxrMaxSources - 1];
  __shared__ double val[3][KD];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int nS = K * D;
  for (int q = tid; q < nS + D; q += 256) {
    if (q < nS)
      S[q] = span_sum(pS + (b * nS + q) * chunks, chunks, 1) / count;
    else
      Nn[q - nS] = span_sum(pN + (b * D + (q - nS)) * chunks, chunks, 1) / count;
  }
  __syncthreads();
  for (int q = tid; q < nS; q += 256) {
    const int k = q / D, d = q - k * D;
    int m = 0;
    for (int n = 0; n < K; ++n)
      if (n != k) others[q][m++] = S[n * D + d];
    I[q] = np_sum(others[q], K - 1, 1);
  }
  __syncthreads();
  // channel means: the reference replaces S, I, N by their means over the last axis
  const int Do = avg_channels ? 1 : D;
  double s_mean = 0.0, i_mean = 0.0, n_mean = 0.0;
  if (avg_channels) {
    if (tid < K) {
      s_mean = np_sum(S + tid * D, D, 1) / (double)D;
      i_mean = np_sum(I + tid * D, D, 1) / (double)D;
    }
    n_mean = np_sum(Nn, D, 1) / (double)D;
  }
  for (int q = tid; q < K * Do; q += 256) {
    const int d = avg_channels ? 0 : q % D;
    const double s = avg_channels ? s_mean : S[q];
    const double i = avg_channels ? i_mean : I[q];
    const double n = avg_channels ? n_mean : Nn[d];
    val[0][q] = sxr_db(s, i + n);
    val[1][q] = sxr_db(s, i);
    val[2][q] = sxr_db(s, n);
  }
  __syncthreads();
  if (!avg_sources) {
    for (int q = tid; q < 3 * K * Do; q += 256) {
      const int m = q / (K * Do);
      out[b * 3 * K * Do + q] = val[m][q - m * K * Do];
    }
  } else {
    for (int q = tid; q < 3 * Do; q += 256) {
      const int m = q / Do, d = q - m * Do;
      double s;
      if (avg_channels) {
        s = np_sum(val[m], K, 1);  // mean of a (K,) array
      } else {
        s = 0.0;  // mean over axis 0 of (K, D): row after row
        for (int k = 0; k < K; ++k) s += val[m][k * D + d];
      }
      out[b * 3 * Do + q] = s / (double)K;
    }
  }
}

// ---- launchers ----------------------------------------------------------------------------
inline int hip_ok() { return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP; }

template <typename T, bool RESID>
void launch_rows_t(const EvalRows& g, int64_t chunks, const double* gram, double* partials,
                   hipStream_t s) {
  const dim3 grid((unsigned)(g.B * chunks)), block(kEvalThreads);
  const int m = g.Kr > g.Ke ? g.Kr : g.Ke;
  if (m <= 1)
    hipLaunchKernelGGL((rows_kernel<T, 1, RESID>), grid, block, 0, s, g, chunks, gram, partials);
  else if (m <= 2)
    hipLaunchKernelGGL((rows_kernel<T, 2, RESID>), grid, block, 0, s, g, chunks, gram, partials);
  else if (m <= 4)
    hipLaunchKernelGGL((rows_kernel<T, 4, RESID>), grid, block, 0, s, g, chunks, gram, partials);
  else
    hipLaunchKernelGGL((rows_kernel<T, 8, RESID>), grid, block, 0, s, g, chunks, gram, partials);
}

template <bool RESID>
void launch_rows(const EvalRows& g, int64_t chunks, const double* gram, double* partials,
                 hipStream_t s) {
  if (g.is_f64)
    launch_rows_t<double, RESID>(g, chunks, gram, partials, s);
  else
    launch_rows_t<float, RESID>(g, chunks, gram, partials, s);
}

// rows of a (possibly complex) array as the Kr = 1, Ke = 0 case of the Gram pass
EvalRows power_rows(const void* x, int dtype, int64_t rows, int64_t length, int64_t row_stride) {
  const int64_t reals = eval_is_complex(dtype) ? 2 : 1;
  EvalRows g{};
  g.ref = x;
  g.est = nullptr;
  g.B = rows;
  g.N = length * reals;
  g.ref_batch = row_stride * reals;
  g.Kr = 1;
  g.Ke = 0;
  g.is_f64 = eval_is_f64(dtype);
  return g;
}

inline unsigned blocks_for(int64_t total) { return (unsigned)((total + 255) / 256); }

}  // namespace

bool eval_grid_ok(int64_t B, int64_t N) {
  const int64_t chunks = eval_chunks(N);
  return B >= 1 && N >= 1 && B <= kEvalMaxWorkgroups / chunks;
}

size_t signal_power_work(int64_t rows, int64_t length, int dtype) {
  return (size_t)rows * (size_t)eval_chunks(length * (eval_is_complex(dtype) ? 2 : 1));
}

size_t si_sdr_work(int64_t B, int Kr, int Ke, int64_t N) {
  const size_t chunks = (size_t)eval_chunks(N);
  // Gram partials, finished Gram, residual partials
  return (size_t)B * ((size_t)(Kr + Kr * Ke) * (chunks + 1) + (size_t)(Kr * Ke) * chunks);
}

int launch_signal_power(const void* x, int dtype, int64_t rows, int64_t length, int64_t row_stride,
                        double* work, double* out, hipStream_t s) {
  const EvalRows g = power_rows(x, dtype, rows, length, row_stride);
  const int64_t chunks = eval_chunks(g.N);
  launch_rows<false>(g, chunks, nullptr, work, s);
  if (out)
    hipLaunchKernelGGL(finish_sum_kernel, dim3(blocks_for(rows)), dim3(256), 0, s, work, rows,
                       chunks, 1, (double)length, out);
  return hip_ok();
}

int launch_si_sdr(const EvalRows& g, double* work, double* out, hipStream_t s) {
  const int64_t chunks = eval_chunks(g.N);
  const int A1 = g.Kr + g.Kr * g.Ke, A2 = g.Kr * g.Ke;
  double* p1 = work;
  double* gram = p1 + g.B * chunks * A1;
  double* p2 = gram + g.B * A1;
  launch_rows<false>(g, chunks, nullptr, p1, s);
  hipLaunchKernelGGL(finish_sum_kernel, dim3(blocks_for(g.B * A1)), dim3(256), 0, s, p1, g.B * A1,
                     chunks, A1, 0.0, gram);
  launch_rows<true>(g, chunks, gram, p2, s);
  hipLaunchKernelGGL(si_sdr_finish_kernel, dim3(blocks_for(g.B * A2)), dim3(256), 0, s, gram, p2,
                     g.B * A2, chunks, g.Kr, g.Ke, out);
  return hip_ok();
}

int launch_output_sxr(const void* contributions, const void* noise, int dtype, int64_t B, int Ks,
                      int Kt, int64_t N, int average_sources, double* work_images,
                      double* work_noise, double* out_sxr, int64_t* out_selection, double* out_mean,
                      hipStream_t s) {
  int rc = launch_signal_power(contributions, dtype, B * Ks * Kt, N, N, work_images, nullptr, s);
  if (rc != PBBSS_OK) return rc;
  rc = launch_signal_power(noise, dtype, B * Kt, N, N, work_noise, nullptr, s);
  if (rc != PBBSS_OK) return rc;
  const int64_t chunks = eval_chunks(N * (eval_is_complex(dtype) ? 2 : 1));
  hipLaunchKernelGGL(output_sxr_kernel, dim3((unsigned)B), dim3(64), 0, s, work_images, work_noise,
                     chunks, (double)N, Ks, Kt, average_sources, out_sxr, out_selection, out_mean);
  return hip_ok();
}

int launch_input_sxr(const void* images, const void* noise, int dtype, int64_t B, int K, int D,
                     int64_t N, int average_sources, int average_channels, double* work_images,
                     double* work_noise, double* out, hipStream_t s) {
  int rc = launch_signal_power(images, dtype, B * K * D, N, N, work_images, nullptr, s);
  if (rc != PBBSS_OK) return rc;
  rc = launch_signal_power(noise, dtype, B * D, N, N, work_noise, nullptr, s);
  if (rc != PBBSS_OK) return rc;
  const int64_t chunks = eval_chunks(N * (eval_is_complex(dtype) ? 2 : 1));
  hipLaunchKernelGGL(input_sxr_kernel, dim3((unsigned)B), dim3(256), 0, s, work_images, work_noise,
                     chunks, (double)N, K, D, average_sources, average_channels, out);
  return hip_ok();
}

}  // namespace pbbss
