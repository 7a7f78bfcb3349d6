// Polyphase resampler and short-time objective intelligibility (reference:
// pb_bss/evaluation/module_stoi.py, which wraps the pystoi package) for gfx950, float64
// throughout.  Per call, all on the caller's stream and without a host read:
//   resample_kernel      one thread per output sample of the Kaiser-windowed sinc, the taps read
//                        from global memory through the cache;
//   stoi_energy_kernel   one wavefront per frame: 20 log10 of the Hann-weighted norm of the
//                        reference row's frames;
//   stoi_select_kernel   one workgroup per row: the maximum, the keep mask, an ordered prefix sum
//                        over tiles of 256 frames -> the source frame of every kept frame and the
//                        kept count;
//   stoi_band_kernel     one workgroup per kFramesPerWg STFT frames of a row pair: each frame of
//                        the compacted signal gathered from its three source frames, x and y
//                        each packed into 256 complex points and transformed side by side
//                        (fft_dev.hpp), |X|^2, the 15 band sums in bin order, sqrt;
//   stoi_segment_kernel  one lane per (segment, band): the clipped, centred, normalised
//                        correlation of 30 + 30 values, one ordered partial per workgroup;
//   stoi_finish_kernel   one wavefront per row: the partials in a fixed order, the mean.
// Only the device knows how many frames a row keeps, so the grids of the last three are sized
// for the most a row of N10 samples can keep and surplus workgroups leave on a uniform test.
// No floating-point atomics: every sum's order is a property of the input alone.
#include "stoi.hpp"
#include "fft_dev.hpp"

#include <math.h>

namespace pbbss {
namespace {

constexpr int kThreads = kStftThreads;       // 256
constexpr int kNfft = 512;
constexpr int kPoints = kNfft / 2;           // complex points of a packed real transform
constexpr int kBins = kPoints + 1;
constexpr double kDynRange = 40.0;
constexpr double kEps = 2.220446049250313e-16;  // np.finfo(float).eps
constexpr double kShort = 1e-5;              // fewer than 30 STFT frames
constexpr double kClip = 6.623413251903491;  // 1 + 10^(15 / 20)

// band i covers the bins [kEdge[i], kEdge[i + 1]): argmin |f - 150 * 2^((2 i -+ 1) / 6)| over
// f = linspace(0, 10000, 513)[:257]; neighbouring bands share their edge
__device__ const int kEdge[kStoiBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109,
                                              138, 174, 219};

// np.hanning(258)[1:-1][j]
__device__ inline double hann(int j) {
  return 0.5 + 0.5 * cospi((double)(2 * (j + 1) - (kStoiFrame + 1)) / (double)(kStoiFrame + 1));
}

__device__ inline int64_t pair_offset(int64_t row, int64_t inner, int64_t so, int64_t si) {
  return (row / inner) * so + (row % inner) * si;
}

// ---- resampler: out[m] = up * sum_n x[n] window[half + m down - n up] ----------------------------
// The lanes of a wavefront start `down` taps apart but each at its own first sample, so that at
// every step they read at most `up` neighbouring taps: one or two cache lines.  (Laying the taps
// out by phase, every lane walking its own row, was measured and loses: DESIGN 4.16.)
template <typename T>
__global__ __launch_bounds__(kThreads) void resample_kernel(const T* __restrict__ x, int64_t N,
                                                            int up, int down,
                                                            const double* __restrict__ window,
                                                            int half, int64_t M,
                                                            double* __restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t row = blockIdx.y;
  if (m >= M) return;
  const int64_t centre = m * down;  // the taps cover n up in [centre - half, centre + half]
  const int64_t lo = centre - half;
  const int64_t n_lo = lo > 0 ? (lo + up - 1) / up : 0;
  int64_t n_hi = (centre + half) / up;
  if (n_hi > N - 1) n_hi = N - 1;
  const int count = n_hi >= n_lo ? (int)(n_hi - n_lo + 1) : 0;
  const T* xr = x + row * N + n_lo;
  // window index half + centre - n up: <= 2 half at n_lo, >= 0 at n_hi
  const double* w = window + (half + centre - n_lo * up);
  double acc = 0.0;
#pragma unroll 4
  for (int i = 0; i < count; ++i) acc = fma((double)xr[i], w[-(int64_t)i * up], acc);
  out[row * M + m] = (double)up * acc;
}

// ---- frame energies of the reference rows: one wavefront per frame -------------------------------
__global__ __launch_bounds__(kThreads) void stoi_energy_kernel(StoiRows g, int F,
                                                               double* __restrict__ energy) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const int64_t row = blockIdx.y;
  if (f >= F) return;  // wave-uniform
  // frame f < F ends at 128 f + 256 < N10
  const double* xr = g.x + pair_offset(row, g.inner, g.x_outer, g.x_inner) + (int64_t)f * kStoiHop;
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < kStoiFrame / 64; ++q) {
    const int j = q * 64 + lane;
    const double v = hann(j) * xr[j];
    acc = fma(v, v, acc);
  }
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if (lane == 0) energy[row * F + f] = 20.0 * log10(sqrt(acc) + kEps);
}

// ---- which frames stay: one workgroup per row ------------------------------------------------------
__global__ __launch_bounds__(kThreads) void stoi_select_kernel(const double* __restrict__ energy,
                                                               int F, int32_t* __restrict__ src,
                                                               int32_t* __restrict__ kept,
                                                               int32_t* __restrict__ out_frames) {
  __shared__ double dscratch[kThreads / 64];
  __shared__ int iscratch[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const double* e = energy + row * F;
  int32_t* s = src + row * F;
  double peak = -INFINITY;
  for (int f = tid; f < F; f += kThreads) peak = fmax(peak, e[f]);
  for (int d = 32; d >= 1; d >>= 1) peak = fmax(peak, __shfl_xor(peak, d, 64));
  if (lane == 0) dscratch[wave] = peak;
  __syncthreads();
  peak = fmax(fmax(dscratch[0], dscratch[1]), fmax(dscratch[2], dscratch[3]));
  int base = 0;
  for (int tile = 0; tile < F; tile += kThreads) {
    const int f = tile + tid;
    const bool keep = f < F && (peak - kDynRange - e[f < F ? f : 0]) < 0.0;
    int v = keep ? 1 : 0;  // inclusive scan over the workgroup
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(v, d, 64);
      if (lane >= d) v += u;
    }
    if (lane == 63) iscratch[wave] = v;
    __syncthreads();
    int before = 0, total = 0;
    for (int i = 0; i < kThreads / 64; ++i) {
      const int c = iscratch[i];
      if (i < wave) before += c;
      total += c;
    }
    __syncthreads();
    if (keep) s[base + before + v - 1] = f;
    base += total;
  }
  if (tid == 0) {
    kept[row] = base;
    if (out_frames) {
      out_frames[2 * row] = F;
      out_frames[2 * row + 1] = base;
    }
  }
}

// ---- third-octave band magnitudes of the compacted signals ------------------------------------------
// STFT frame t of the compacted signal, sample i: the overlap-add of the windowed kept frames
// k = t - 1, t, t + 1 (source frames src[k]), windowed again:
//   i <  128: (w[128 + i] x[128 src[t - 1] + 128 + i] (t >= 1) + w[i] x[128 src[t] + i]) w[i]
//   i >= 128: (w[i] x[128 src[t] + i] + w[i - 128] x[128 src[t + 1] + i - 128]) w[i]
// Threads 0..127 take x, 128..255 y; each packs two neighbouring samples into one complex point.
__global__ __launch_bounds__(kThreads) void stoi_band_kernel(StoiRows g, int F, int Tmax,
                                                             const int32_t* __restrict__ src,
                                                             const int32_t* __restrict__ kept,
                                                             double* __restrict__ tob) {
  __shared__ Cplx bufa[2 * kPoints], bufb[2 * kPoints], roots[kBins];
  __shared__ double win[kStoiFrame], power[2][kBins + 3];
  const int tid = threadIdx.x, sig = tid >> 7, j = tid & 127;
  const int64_t row = blockIdx.y;
  const int T = kept[row] - 1;
  const int t0 = blockIdx.x * kFramesPerWg;
  if (t0 >= T) return;  // uniform
  build_roots(roots, kNfft, tid);
  win[tid] = hann(tid);
  const double* p = sig ? g.y + pair_offset(row, g.inner, g.y_outer, g.y_inner)
                        : g.x + pair_offset(row, g.inner, g.x_outer, g.x_inner);
  const int32_t* s = src + row * F;
  const int i0 = 2 * j, lower = i0 < kStoiHop;  // both samples lie in the same half of the frame
  for (int ft = 0; ft < kFramesPerWg; ++ft) {
    const int t = t0 + ft;
    if (t >= T) break;  // uniform
    __syncthreads();    // roots and window ready / the previous frame consumed
    {
#pragma clang fp contract(off)
      // loads at clamped indices, the mask afterwards; t + 1 <= T = kept - 1
      const bool first = lower && t == 0;
      const int ka = lower ? (first ? 0 : t - 1) : t, kb = lower ? t : t + 1;
      const int ia = lower ? i0 + kStoiHop : i0, ib = lower ? i0 : i0 - kStoiHop;
      const int64_t oa = (int64_t)s[ka] * kStoiHop + ia, ob = (int64_t)s[kb] * kStoiHop + ib;
      const double a0 = p[oa], a1 = p[oa + 1], b0 = p[ob], b1 = p[ob + 1];
      const double wa0 = win[ia], wa1 = win[ia + 1], wb0 = win[ib], wb1 = win[ib + 1];
      const double u0 = first ? 0.0 : wa0 * a0, u1 = first ? 0.0 : wa1 * a1;
      const double c0 = u0 + wb0 * b0, c1 = u1 + wb1 * b1;
      bufa[sig * kPoints + j] = {c0 * win[i0], c1 * win[i0 + 1]};
      bufa[sig * kPoints + 128 + j] = {0.0, 0.0};  // samples 256..511 of the transform
    }
    __syncthreads();
    const Cplx* Z = stockham<-1>(bufa + sig * kPoints, bufb + sig * kPoints, roots, kPoints, j);
    // untangle: X[k] = Xe + exp(-2 pi i k / 512) Xo from the even / odd sample spectra
    for (int k = j; k < kBins; k += 128) {
      const Cplx zk = Z[k & (kPoints - 1)], zc = Z[(kPoints - k) & (kPoints - 1)];
      const Cplx xe = {0.5 * (zk.re + zc.re), 0.5 * (zk.im - zc.im)};
      const Cplx xo = {0.5 * (zk.im + zc.im), -0.5 * (zk.re - zc.re)};
      const Cplx r = cmul(roots[k], xo);
      const double re = xe.re + r.re, im = xe.im + r.im;
      power[sig][k] = re * re + im * im;
    }
    __syncthreads();
    if (tid < 2 * kStoiBands) {
      const int which = tid / kStoiBands, band = tid % kStoiBands;
      double acc = 0.0;
      for (int k = kEdge[band]; k < kEdge[band + 1]; ++k) acc += power[which][k];
      tob[((row * 2 + which) * Tmax + t) * kStoiBands + band] = sqrt(acc);
    }
  }
}

// ---- segments: one lane per (segment, band) ------------------------------------------------------------
__device__ inline double norm30(const double (&v)[kStoiSegment]) {
  double acc = 0.0;
#pragma unroll
  for (int s = 0; s < kStoiSegment; ++s) acc = fma(v[s], v[s], acc);
  return sqrt(acc);
}

__device__ inline void centre30(double (&v)[kStoiSegment]) {
  double sum = 0.0;
#pragma unroll
  for (int s = 0; s < kStoiSegment; ++s) sum += v[s];
  const double mean = sum / (double)kStoiSegment;
#pragma unroll
  for (int s = 0; s < kStoiSegment; ++s) v[s] -= mean;
}

__global__ __launch_bounds__(kStoiSegThreads) void stoi_segment_kernel(
    const double* __restrict__ tob, int Tmax, int Pmax, const int32_t* __restrict__ kept,
    double* __restrict__ partial) {
  __shared__ double scratch[kStoiSegThreads / 64];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.y;
  const int items = (kept[row] - 1 - (kStoiSegment - 1)) * kStoiBands;
  const int first = blockIdx.x * kStoiSegThreads;
  if (first >= items) return;  // uniform; also every row with fewer than 30 frames
  const bool active = first + tid < items;
  // item i = segment * 15 + band starts at tob[i] and steps one frame (15 doubles) at a time
  const int i = active ? first + tid : first;
  const double* xt = tob + (row * 2 + 0) * Tmax * kStoiBands + i;
  const double* yt = tob + (row * 2 + 1) * Tmax * kStoiBands + i;
  double xs[kStoiSegment], ys[kStoiSegment];
#pragma unroll
  for (int s = 0; s < kStoiSegment; ++s) {
    xs[s] = xt[s * kStoiBands];
    ys[s] = yt[s * kStoiBands];
  }
  const double c = norm30(xs) / (norm30(ys) + kEps);
#pragma unroll
  for (int s = 0; s < kStoiSegment; ++s) {
    const double scaled = ys[s] * c, bound = xs[s] * kClip;
    ys[s] = scaled < bound ? scaled : bound;
  }
  centre30(xs);
  centre30(ys);
  const double nx = norm30(xs) + kEps, ny = norm30(ys) + kEps;
  double d = 0.0;
#pragma unroll
  for (int s = 0; s < kStoiSegment; ++s) d = fma(ys[s] / ny, xs[s] / nx, d);
  if (!active) d = 0.0;
  for (int w = 32; w >= 1; w >>= 1) d += __shfl_xor(d, w, 64);
  if ((tid & 63) == 0) scratch[tid >> 6] = d;
  __syncthreads();
  if (tid == 0)
    partial[row * Pmax + blockIdx.x] = ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

// ---- the mean over segments and bands: one wavefront per row ----------------------------------------
__global__ __launch_bounds__(64) void stoi_finish_kernel(const double* __restrict__ partial,
                                                         int Pmax,
                                                         const int32_t* __restrict__ kept,
                                                         double* __restrict__ out) {
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int J = kept[row] - 1 - (kStoiSegment - 1);
  if (J < 1) {  // uniform
    if (lane == 0) out[row] = kShort;
    return;
  }
  const int items = J * kStoiBands;
  const int P = (items + kStoiSegThreads - 1) / kStoiSegThreads;
  double acc = 0.0;
  for (int q = lane; q < P; q += 64) acc += partial[row * Pmax + q];
  for (int w = 32; w >= 1; w >>= 1) acc += __shfl_xor(acc, w, 64);
  if (lane == 0) out[row] = acc / (double)items;
}

inline int hip_ok() { return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP; }

}  // namespace

int launch_resample_poly(const void* x, int is_f64, int64_t rows, int64_t N, int up, int down,
                         const double* window, int half, double* out, hipStream_t s) {
  const int64_t M = resample_length(N, up, down);
  const dim3 grid((unsigned)((M + kThreads - 1) / kThreads), (unsigned)rows), block(kThreads);
  if (is_f64)
    hipLaunchKernelGGL(resample_kernel<double>, grid, block, 0, s, static_cast<const double*>(x),
                       N, up, down, window, half, M, out);
  else
    hipLaunchKernelGGL(resample_kernel<float>, grid, block, 0, s, static_cast<const float*>(x), N,
                       up, down, window, half, M, out);
  return hip_ok();
}

int launch_stoi(const StoiRows& g, const StoiWork& w, double* out, int32_t* out_frames,
                hipStream_t s) {
  const int64_t rows = g.outer * g.inner;
  const int F = (int)stoi_frames(g.N10), Tmax = (int)stoi_max_stft_frames(g.N10);
  const int Pmax = (int)stoi_max_partials(g.N10);
  if (F > 0)
    hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)((F + 3) / 4), (unsigned)rows),
                       dim3(kThreads), 0, s, g, F, w.energy);
  hipLaunchKernelGGL(stoi_select_kernel, dim3((unsigned)rows), dim3(kThreads), 0, s, w.energy, F,
                     w.src, w.kept, out_frames);
  if (Pmax > 0) {  // a row can reach 30 STFT frames
    hipLaunchKernelGGL(stoi_band_kernel,
                       dim3((unsigned)((Tmax + kFramesPerWg - 1) / kFramesPerWg), (unsigned)rows),
                       dim3(kThreads), 0, s, g, F, Tmax, w.src, w.kept, w.tob);
    hipLaunchKernelGGL(stoi_segment_kernel, dim3((unsigned)Pmax, (unsigned)rows),
                       dim3(kStoiSegThreads), 0, s, w.tob, Tmax, Pmax, w.kept, w.partial);
  }
  hipLaunchKernelGGL(stoi_finish_kernel, dim3((unsigned)rows), dim3(64), 0, s, w.partial, Pmax,
                     w.kept, out);
  return hip_ok();
}

}  // namespace pbbss
