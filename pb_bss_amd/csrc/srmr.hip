// Gammatone filterbank and SRMR (reference: pb_bss/transform/gammatone.py,
// pb_bss/evaluation/module_srmr.py) for gfx950, float64 throughout.
//
// Every filter of the reference is a biquad, a serial recurrence over the samples of a row.  The
// recurrence is linear, so it is split along time: one wavefront owns one recurrence, its 64
// lanes take 64 consecutive chunks of kBiquadChunk samples (one tile), and tile follows tile with
// the filter state handed on.  Per tile (biquad_chunked):
//   1. every lane runs its chunk from a zero state and keeps the end state e = (z1, z2);
//   2. the true end states S_l = e_l + A^L S_(l-1) (A: the 2 x 2 state matrix of the homogeneous
//      recurrence, L the chunk length, S_(-1) the state carried in from the previous tile) come
//      from a six-step scan over the lanes with the lane-uniform matrices A^(L 2^k);
//   3. every lane runs its chunk again from S_(l-1).  By linearity that is the zero-state response
//      plus the homogeneous response s1 h1[t] + s2 h2[t] of the carried state, formed in the
//      recurrence's own registers: no table of h1 / h2, no second trip through LDS, and the
//      rounding of the serial filter except for the carry.
// Samples at or beyond a row's length are zeros in the tile and are never read from memory.
#include "srmr.hpp"

#include <math.h>

namespace pbbss {
namespace {

constexpr int L = kBiquadChunk;
constexpr int kPitch = L + 1;         // doubles between two chunks in LDS: lanes l, l + 32 share a
                                      // bank and lie in different halves of a 64-bit access
constexpr int kTileLds = 64 * kPitch;
constexpr int kPowers = 6;            // A^(L 2^k), k = 0 .. 5: one per step of the lane scan
constexpr int kVadThreads = 1024;

struct Biquad {
  double b0, b1, b2, a1, a2;
};

__device__ inline Biquad load_biquad(const double* c) { return Biquad{c[0], c[1], c[2], c[3], c[4]}; }

// Double-double arithmetic for the matrix powers below: an unevaluated sum hi + lo, |lo| <= ulp(hi) / 2.
// Contraction is switched off inside: the error terms rely on p being the ROUNDED product wherever
// it is used.  A compiler that fuses a.hi * b.hi into some of its uses (p + e, s - p) and not into
// others counts the product's rounding error twice and leaves plain float64 accuracy behind.
struct DD {
  double hi, lo;
};
__device__ inline DD dd_mul(DD a, DD b) {
#pragma clang fp contract(off)
  const double p = a.hi * b.hi;
  double e = fma(a.hi, b.hi, -p);
  e = fma(a.hi, b.lo, e);
  e = fma(a.lo, b.hi, e);
  const double s = p + e;
  return DD{s, e - (s - p)};
}
__device__ inline DD dd_add(DD a, DD b) {
#pragma clang fp contract(off)
  const double s = a.hi + b.hi, v = s - a.hi;
  const double e = ((a.hi - (s - v)) + (b.hi - v)) + (a.lo + b.lo);
  const double h = s + e;
  return DD{h, e - (h - s)};
}

// pw[4 k .. 4 k + 3] = A^(L 2^k) row-major, A = [[-a1, 1], [-a2, 0]].  Lane-uniform arithmetic;
// the caller lets one lane store.  The powers come from repeated squaring, eleven times for the
// last one, and a squaring doubles the relative error it is handed.  The modulation filters at
// 4 and 6.5 Hz have both poles within 0.003 of z = 1, where the entries of A^k cancel by a factor
// of several hundred: in plain float64 the powers cost 5e-9 of the band energy (measured on the
// host), in double-double, rounded once at the end, nothing that shows.
__device__ inline void biquad_powers(const Biquad& q, double* pw, bool store) {
  DD m00{-q.a1, 0.0}, m01{1.0, 0.0}, m10{-q.a2, 0.0}, m11{0.0, 0.0};
  int squarings = 0;
  for (int c = L; c > 1; c >>= 1) ++squarings;
  for (int i = 0; i < squarings + kPowers; ++i) {
    if (i >= squarings && store) {
      double* p = pw + 4 * (i - squarings);
      p[0] = m00.hi, p[1] = m01.hi, p[2] = m10.hi, p[3] = m11.hi;
    }
    const DD n00 = dd_add(dd_mul(m00, m00), dd_mul(m01, m10));
    const DD n01 = dd_add(dd_mul(m00, m01), dd_mul(m01, m11));
    const DD n10 = dd_add(dd_mul(m10, m00), dd_mul(m11, m10));
    const DD n11 = dd_add(dd_mul(m10, m01), dd_mul(m11, m11));
    m00 = n00, m01 = n01, m10 = n10, m11 = n11;
  }
}

// direct form II transposed, one sample
__device__ inline double biquad_step(const Biquad& q, double x, double& z1, double& z2) {
  const double y = fma(q.b0, x, z1);
  z1 = fma(-q.a1, y, fma(q.b1, x, z2));
  z2 = fma(-q.a2, y, q.b2 * x);
  return y;
}

// One wavefront, one recurrence, one tile.  `chunk`: the calling lane's L samples in LDS; (g1, g2):
// the state at the start of the tile, advanced to the start of the next one; pw: biquad_powers of
// q in LDS.  sink(t, y) receives the output sample t of the lane's chunk.
template <typename Sink>
__device__ inline void biquad_chunked(const Biquad& q, const double* pw, const double* chunk,
                                      int lane, double& g1, double& g2, Sink&& sink) {
  double e1 = 0.0, e2 = 0.0;
#pragma unroll 8
  for (int t = 0; t < L; ++t) (void)biquad_step(q, chunk[t], e1, e2);
  if (lane == 0) {  // the carried state enters through the first chunk
    e1 += pw[0] * g1 + pw[1] * g2;
    e2 += pw[2] * g1 + pw[3] * g2;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int d = 1 << k;
    const double u1 = __shfl_up(e1, d, 64), u2 = __shfl_up(e2, d, 64);
    if (lane >= d) {
      const double* p = pw + 4 * k;
      e1 += p[0] * u1 + p[1] * u2;
      e2 += p[2] * u1 + p[3] * u2;
    }
  }
  double z1 = __shfl_up(e1, 1, 64), z2 = __shfl_up(e2, 1, 64);
  if (lane == 0) z1 = g1, z2 = g2;
  g1 = __shfl(e1, 63, 64);
  g2 = __shfl(e2, 63, 64);
#pragma unroll 8
  for (int t = 0; t < L; ++t) sink(t, biquad_step(q, chunk[t], z1, z2));
}

__device__ inline int clamp_length(const int32_t* lengths, int64_t row, int64_t N) {
  int64_t len = lengths ? (int64_t)lengths[row] : N;
  if (len < 0) len = 0;
  if (len > N) len = N;
  return (int)len;
}

// ---- gammatone filterbank: one wavefront per (row, channel), the four stages in place ----------
template <typename T>
__global__ __launch_bounds__(64) void gammatone_kernel(const T* __restrict__ x, int64_t rows,
                                                       int64_t N, const int32_t* lengths, int n,
                                                       const double* __restrict__ coef,
                                                       double* __restrict__ out) {
  __shared__ double tile[kTileLds];
  __shared__ double pw[kGammatoneStages][4 * kPowers];
  const int lane = threadIdx.x;
  const int ch = (int)(blockIdx.x % (unsigned)n);
  const int64_t row = blockIdx.x / (unsigned)n;
  const int len = clamp_length(lengths, row, N);
  Biquad q[kGammatoneStages];
  double g[kGammatoneStages][2];
  for (int s = 0; s < kGammatoneStages; ++s) {
    q[s] = load_biquad(coef + ((int64_t)ch * kGammatoneStages + s) * kBiquadCoefs);
    biquad_powers(q[s], pw[s], lane == 0);
    g[s][0] = g[s][1] = 0.0;
  }
  __syncthreads();
  const T* xr = x + row * N;
  double* o = out + ((int64_t)ch * rows + row) * N;
  double* chunk = tile + lane * kPitch;
  for (int base = 0; base < len; base += kBiquadTile) {
#pragma unroll 4
    for (int j = 0; j < L; ++j) {  // sample base + 64 j + lane: chunk (64 j + lane) / L
      const int i = j * 64 + lane, t = base + i;
      tile[(i / L) * kPitch + i % L] = t < len ? (double)xr[t] : 0.0;
    }
    __syncthreads();
    for (int s = 0; s < kGammatoneStages; ++s)
      biquad_chunked(q[s], pw[s], chunk, lane, g[s][0], g[s][1],
                     [&](int t, double y) { chunk[t] = y; });
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < L; ++j) {
      const int i = j * 64 + lane, t = base + i;
      if (t < len) o[t] = tile[(i / L) * kPitch + i % L];
    }
    __syncthreads();
  }
  for (int64_t t = (int64_t)len + lane; t < N; t += 64) o[t] = 0.0;
}

// ---- frame weight: W[t] = sum over the frames f that hold t of hamming(t - f hop)^2 ------------
// F = max(ceil((len - flen) / hop), 0) + 1 frames, the last one zero-padded.
__device__ inline int srmr_frames(int len, int flen, int hop) {
  const int d = len - flen;
  return d > 0 ? (d + hop - 1) / hop + 1 : 1;
}

__global__ __launch_bounds__(256) void srmr_weight_kernel(int64_t N, const int32_t* lengths,
                                                          int flen, int hop,
                                                          double* __restrict__ W) {
  const int64_t row = blockIdx.y;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N) return;
  const int len = clamp_length(lengths, row, N);
  double w = 0.0;
  if (t < len) {
    const int F = srmr_frames(len, flen, hop);
    int f_hi = (int)(t / hop);
    if (f_hi > F - 1) f_hi = F - 1;
    const int f_lo = t >= flen ? (int)((t - flen) / hop) + 1 : 0;
    const double step = 2.0 * M_PI / (double)(flen - 1);
    for (int f = f_lo; f <= f_hi; ++f) {
      const double ham = 0.54 + 0.46 * cos(fma((double)(t - (int64_t)f * hop), step, -M_PI));
      w = fma(ham, ham, w);
    }
  }
  W[row * N + t] = w;
}

// ---- modulation energies: one workgroup per (row, channel), one wavefront per modulation filter --
__global__ __launch_bounds__(64 * kSrmrModFilters) void srmr_energy_kernel(
    const double2* __restrict__ analytic, const double* __restrict__ W, int64_t rows, int64_t N,
    const int32_t* lengths, int n, int flen, int hop, const double* __restrict__ coef,
    double* __restrict__ means) {
  __shared__ double env[kTileLds];
  __shared__ double wt[kTileLds];
  __shared__ double pw[kSrmrModFilters][4 * kPowers];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ch = (int)(blockIdx.x % (unsigned)n);
  const int64_t row = blockIdx.x / (unsigned)n;
  const int len = clamp_length(lengths, row, N);
  const Biquad q = load_biquad(coef + wave * kBiquadCoefs);
  biquad_powers(q, pw[wave], lane == 0);
  const double2* a = analytic + ((int64_t)ch * rows + row) * N;
  const double* w = W + row * N;
  double g1 = 0.0, g2 = 0.0, acc = 0.0;
  const double* chunk = env + lane * kPitch;
  const double* wchunk = wt + lane * kPitch;
  for (int base = 0; base < len; base += kBiquadTile) {
    __syncthreads();  // the previous tile is consumed (first pass: the powers are stored)
    for (int i = threadIdx.x; i < kBiquadTile; i += 64 * kSrmrModFilters) {
      const int t = base + i;
      double e = 0.0, wv = 0.0;
      if (t < len) {
        const double2 v = a[t];
        e = sqrt(v.x * v.x + v.y * v.y);
        wv = w[t];
      }
      const int at = (i / L) * kPitch + i % L;
      env[at] = e;
      wt[at] = wv;
    }
    __syncthreads();
    biquad_chunked(q, pw[wave], chunk, lane, g1, g2,
                   [&](int t, double y) { acc = fma(wchunk[t] * y, y, acc); });
  }
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if (lane == 0)
    means[(row * n + ch) * kSrmrModFilters + wave] = acc / (double)srmr_frames(len, flen, hop);
}

// ---- scalar tail (module_srmr.py:104-154): one lane per row --------------------------------------
__global__ __launch_bounds__(64) void srmr_score_kernel(const double* __restrict__ means,
                                                        int64_t rows, int n,
                                                        const double* __restrict__ erbs,
                                                        const double* __restrict__ cutoffs,
                                                        double* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= rows) return;
  const double* m = means + row * n * kSrmrModFilters;
  double col[kSrmrModFilters] = {};
  double total = 0.0;
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < kSrmrModFilters; ++k) {
      col[k] += m[j * kSrmrModFilters + k];
      total += m[j * kSrmrModFilters + k];
    }
  double cumulative = 0.0, bandwidth = 0.0;
  for (int j = 0; j < n; ++j) {
    double channel = 0.0;
    for (int k = 0; k < kSrmrModFilters; ++k) channel += m[j * kSrmrModFilters + k];
    cumulative += channel * 100.0 / total;
    if (cumulative > 90.0) {
      bandwidth = erbs[j];
      break;
    }
  }
  const double numerator = col[0] + col[1] + col[2] + col[3];
  double denominator = col[4];
  for (int i = 5; i < kSrmrModFilters; ++i) {
    denominator += col[i];
    if (cutoffs[i - 1] < bandwidth && bandwidth < cutoffs[i]) break;
  }
  out[row] = numerator / denominator;
}

// ---- voice activity detection and normalisation: one workgroup per row ----------------------------
struct OpMin {
  static constexpr int identity = INT32_MAX;
  __device__ static int apply(int a, int b) { return a < b ? a : b; }
};
struct OpMax {
  static constexpr int identity = -1;
  __device__ static int apply(int a, int b) { return a > b ? a : b; }
};
struct OpAdd {
  static constexpr int identity = 0;
  __device__ static int apply(int a, int b) { return a + b; }
};

// inclusive scan over the kVadThreads lanes of the workgroup; *total: the scan's last element.
// scratch: kVadThreads / 64 ints.  Ends with the scratch free for the next call.
template <typename Op>
__device__ inline int block_scan(int v, int* scratch, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v = Op::apply(u, v);
  }
  if (lane == 63) scratch[wave] = v;
  __syncthreads();
  int before = Op::identity, all = Op::identity;
  for (int i = 0; i < kVadThreads / 64; ++i) {
    const int s = scratch[i];
    if (i < wave) before = Op::apply(before, s);
    all = Op::apply(all, s);
  }
  __syncthreads();
  *total = all;
  return Op::apply(before, v);
}

template <bool kMax>
__device__ inline double block_reduce(double v, double* scratch) {
  for (int d = 32; d >= 1; d >>= 1) {
    const double u = __shfl_xor(v, d, 64);
    v = kMax ? fmax(v, u) : v + u;
  }
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = scratch[0];
  for (int i = 1; i < kVadThreads / 64; ++i) r = kMax ? fmax(r, scratch[i]) : r + scratch[i];
  __syncthreads();
  return r;
}

template <typename T>
__global__ __launch_bounds__(kVadThreads) void srmr_vad_kernel(const T* __restrict__ x, int64_t N64,
                                                               double width, int32_t* right_ws,
                                                               double* out, int32_t* out_lengths) {
  __shared__ int iscratch[kVadThreads / 64];
  __shared__ double dscratch[kVadThreads / 64];
  const int N = (int)N64;  // N <= 2^24
  const int64_t row = blockIdx.x;
  const T* xr = x + row * N64;
  int32_t* right = right_ws + row * N64;
  double* o = out + row * N64;
  const int tid = threadIdx.x;

  double peak = 0.0;
  for (int t = tid; t < N; t += kVadThreads) peak = fmax(peak, fabs((double)xr[t]));
  peak = block_reduce<true>(peak, dscratch);
  const double threshold = peak * peak / 1e5;  // compared with |x|, as the reference does

  // backwards: the nearest flagged index at or after every sample (lane order reversed in time)
  const int tiles = (N + kVadThreads - 1) / kVadThreads;
  int carry = INT32_MAX;
  for (int tile = tiles - 1; tile >= 0; --tile) {
    const int t = tile * kVadThreads + (kVadThreads - 1 - tid);
    const bool flag = t < N && fabs((double)xr[t]) > threshold;
    int total;
    const int nearest = block_scan<OpMin>(flag ? t : INT32_MAX, iscratch, &total);
    if (t < N) right[t] = OpMin::apply(nearest, carry);
    carry = OpMin::apply(carry, total);
  }
  __syncthreads();

  // forwards: the nearest flagged index at or before, the decision, the compaction
  int left_carry = -1, kept = 0;
  for (int tile = 0; tile < tiles; ++tile) {
    const int t = tile * kVadThreads + tid;
    const bool inside = t < N;
    const double v = inside ? (double)xr[t] : 0.0;
    const bool flag = inside && fabs(v) > threshold;
    int total;
    int left = block_scan<OpMax>(flag ? t : -1, iscratch, &total);
    left = OpMax::apply(left, left_carry);
    left_carry = OpMax::apply(left_carry, total);
    bool keep = inside;
    if (inside && !flag) {
      const int r = right[t];
      if (left >= 0 && r != INT32_MAX && (double)(r - left) > width) keep = false;
    }
    const int position = block_scan<OpAdd>(keep ? 1 : 0, iscratch, &total);
    if (keep) o[kept + position - 1] = v;
    kept += total;
  }
  __syncthreads();

  // x - mean, then / std of the centred signal (ddof = 0), as NumPy evaluates the two lines
  const double count = (double)kept;
  double sum = 0.0;
  for (int t = tid; t < kept; t += kVadThreads) sum += o[t];
  const double mean = block_reduce<false>(sum, dscratch) / count;
  sum = 0.0;
  for (int t = tid; t < kept; t += kVadThreads) sum += o[t] - mean;
  const double mean2 = block_reduce<false>(sum, dscratch) / count;
  sum = 0.0;
  for (int t = tid; t < kept; t += kVadThreads) {
    const double d = (o[t] - mean) - mean2;
    sum = fma(d, d, sum);
  }
  const double deviation = sqrt(block_reduce<false>(sum, dscratch) / count);
  for (int t = tid; t < N; t += kVadThreads) o[t] = t < kept ? (o[t] - mean) / deviation : 0.0;
  if (tid == 0) out_lengths[row] = kept;
}

inline int hip_ok() { return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP; }

}  // namespace

int launch_srmr_vad(const void* x, int is_f64, int64_t rows, int64_t N, int sample_rate,
                    int32_t* right_ws, double* out, int32_t* out_lengths, hipStream_t s) {
  const double width = 0.05 * (double)sample_rate;
  const dim3 grid((unsigned)rows), block(kVadThreads);
  if (is_f64)
    hipLaunchKernelGGL(srmr_vad_kernel<double>, grid, block, 0, s, static_cast<const double*>(x), N,
                       width, right_ws, out, out_lengths);
  else
    hipLaunchKernelGGL(srmr_vad_kernel<float>, grid, block, 0, s, static_cast<const float*>(x), N,
                       width, right_ws, out, out_lengths);
  return hip_ok();
}

int launch_gammatone(const void* x, int is_f64, int64_t rows, int64_t N, const int32_t* lengths,
                     int n, const double* coef, double* out, hipStream_t s) {
  const dim3 grid((unsigned)(rows * n)), block(64);
  if (is_f64)
    hipLaunchKernelGGL(gammatone_kernel<double>, grid, block, 0, s, static_cast<const double*>(x),
                       rows, N, lengths, n, coef, out);
  else
    hipLaunchKernelGGL(gammatone_kernel<float>, grid, block, 0, s, static_cast<const float*>(x),
                       rows, N, lengths, n, coef, out);
  return hip_ok();
}

int launch_srmr_energies(const void* analytic, int64_t rows, int64_t N, const int32_t* lengths,
                         int n, int sample_rate, const double* coef, double* weights,
                         double* out_means, hipStream_t s) {
  const int flen = srmr_frame_length(sample_rate), hop = srmr_frame_hop(sample_rate);
  hipLaunchKernelGGL(srmr_weight_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)rows),
                     dim3(256), 0, s, N, lengths, flen, hop, weights);
  hipLaunchKernelGGL(srmr_energy_kernel, dim3((unsigned)(rows * n)), dim3(64 * kSrmrModFilters), 0,
                     s, static_cast<const double2*>(analytic), weights, rows, N, lengths, n, flen,
                     hop, coef, out_means);
  return hip_ok();
}

int launch_srmr_score(const double* means, int64_t rows, int n, const double* erbs,
                      const double* cutoffs, double* out, hipStream_t s) {
  hipLaunchKernelGGL(srmr_score_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, s, means,
                     rows, n, erbs, cutoffs, out);
  return hip_ok();
}

}  // namespace pbbss
