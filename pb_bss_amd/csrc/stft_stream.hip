// Streaming STFT / inverse STFT (include/pbbss_stream.h): the two ends of the frame-recursive
// chain.  A block of samples in -> the frames it completes; a block of frames in -> the hops they
// complete; one launch per call, the state in tensors of the caller, and any blocking gives bit
// for bit what stft.hip gives for the whole signal.
//
// Forward: stft_kernel with another source of samples.  One 256-thread workgroup transforms
// kFramesPerWg consecutive frames of one channel; windowing, FFT (fft_dev.hpp) and untangling are
// the statements of stft_kernel, so a frame is bitwise the offline one.  A sample is addressed by
// its position r relative to the first sample of the block: r >= 0 lies in the block, r < 0 in the
// history (C, hist_len) float64 that the previous call left.  The same launch writes the history
// behind the block into a SECOND buffer (the host flips the roles), so no workgroup has to wait
// for another: every one reads the old history, workgroup x = 0 of a channel writes the new one.
//
// Inverse: one workgroup per row walks the m frames of the call in order.  The overlap tail lives
// in LDS as a ring of window_length float64 sums; per frame: inverse FFT, synthesis window, add
// into the ring, emit the oldest hop and clear its slots.  A sum therefore starts from 0.0 and
// takes its covering frames in ascending order, exactly as istft_ola_kernel adds them, whatever
// the blocking; the tail goes back to HBM once, at the end of the call.  No scratch in HBM.
// The serial walk costs m dependent FFTs per row and fills rows compute units only: right for the
// few frames and rows of a streaming call (DESIGN.md 4.22 has the figures for large m).
//
// The product irfft * window is rounded BEFORE it is added (the offline kernel stores it to
// scratch in between): add_rounded_product keeps the compiler from contracting the two.
#include "stft_stream.hpp"
#include "fft_dev.hpp"
#include "launch_util.hpp"
#include <cmath>
#include "pbbss_dev.hpp"

namespace pbbss {
namespace {

// sample at position r in [-hist_len, n): unconditional loads at clamped indices from both
// sources, the choice afterwards
__device__ __forceinline__ double stream_sample(const StftStreamArgs& g, const double* hist,
                                                int64_t c, int64_t r) {
  int64_t bi = r < 0 ? 0 : r;
  if (bi > g.n - 1) bi = g.n - 1;
  if (bi < 0) bi = 0;
  int64_t hi = g.hist_len + r;
  if (hi < 0) hi = 0;
  if (hi > g.hist_len - 1) hi = g.hist_len - 1;
  const double hv = hist[hi];
  double bv;
  if (g.x_is_f64) {
    bv = static_cast<const double*>(g.x)[c * g.n + bi];
  } else {
    const float f = static_cast<const float*>(g.x)[c * g.n + bi];
    bv = (double)f;
  }
  return r >= 0 ? bv : hv;
}

__global__ void __launch_bounds__(kStftThreads) stft_stream_kernel(StftStreamArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int N = g.size, M = N / 2, F = M + 1;
  Cplx* bufa = reinterpret_cast<Cplx*>(smem);
  Cplx* bufb = bufa + M;
  Cplx* roots = bufb + M;  // [M + 1]
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.y;
  const double* hist = g.hist_in + c * g.hist_len;
  if (blockIdx.x == 0) {  // the history behind the block: the last hist_len samples seen
    double* ho = g.hist_out + c * g.hist_len;
    for (int j = tid; j < g.hist_len; j += kStftThreads) {
      const double v = stream_sample(g, hist, c, (int64_t)j - g.hist_len + g.n);
      ho[j] = g.reset ? 0.0 : v;
    }
  }
  build_roots(roots, N, tid);
  for (int ft = 0; ft < kFramesPerWg; ++ft) {
    const int t = blockIdx.x * kFramesPerWg + ft;
    if (t >= g.m) break;  // uniform
    __syncthreads();      // roots ready / previous frame fully written out
    const int64_t s0 = g.base + (int64_t)t * g.shift;
    for (int n = tid; n < M; n += kStftThreads) {
      bool ok[2];
      int64_t rc[2];
      int wc[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int m = 2 * n + h;
        const int64_t r = s0 + m;
        ok[h] = m < g.wl && r >= g.lo && r < g.n;
        rc[h] = ok[h] ? r : g.lo;
        wc[h] = ok[h] ? m : 0;
      }
      double xv[2], wv[2];
      xv[0] = stream_sample(g, hist, c, rc[0]);
      xv[1] = stream_sample(g, hist, c, rc[1]);
      wv[0] = g.window[wc[0]];
      wv[1] = g.window[wc[1]];
      bufa[n] = {ok[0] ? xv[0] * wv[0] : 0.0, ok[1] ? xv[1] * wv[1] : 0.0};
    }
    __syncthreads();
    const Cplx* Z = stockham<-1>(bufa, bufb, roots, M, tid);
    // untangle: X[k] = Xe + exp(-2 pi i k / N) Xo with the even / odd sample spectra
    // Xe = (Z[k] + conj Z[M-k]) / 2, Xo = (Z[k] - conj Z[M-k]) / (2i)
    for (int k = tid; k < F; k += kStftThreads) {
      const Cplx zk = Z[k & (M - 1)], zc = Z[(M - k) & (M - 1)];
      const Cplx xe = {0.5 * (zk.re + zc.re), 0.5 * (zk.im - zc.im)};
      const Cplx xo = {0.5 * (zk.im + zc.im), -0.5 * (zk.re - zc.re)};
      const Cplx r = cmul(roots[k], xo);
      const double ore = xe.re + r.re, oim = xe.im + r.im;
      const size_t idx = (g.layout == 0) ? ((size_t)c * g.m + t) * F + k
                                         : ((size_t)k * g.m + t) * g.C + c;
      if (g.out_c128) {
        double* o = static_cast<double*>(g.out) + 2 * idx;
        o[0] = ore;
        o[1] = oim;
      } else {
        float* o = static_cast<float*>(g.out) + 2 * idx;
        o[0] = (float)ore;
        o[1] = (float)oim;
      }
    }
  }
}

// acc + (a * scale * w) with the product rounded on its own: the empty statement makes the
// product opaque, so no fused multiply-add can take the place of the multiply and the add
__device__ __forceinline__ double add_rounded_product(double acc, double a, double scale, double w) {
  double p = a * scale * w;
  asm volatile("" : "+v"(p));
  return acc + p;
}

__global__ void __launch_bounds__(kStftThreads) istft_stream_kernel(IstftStreamArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int N = g.size, M = N / 2, F = M + 1;
  Cplx* bufa = reinterpret_cast<Cplx*>(smem);
  Cplx* bufb = bufa + M;
  Cplx* spec = bufb;            // [F] the frame's spectrum: bufb and one more entry, dead before
  Cplx* roots = bufb + M + 1;   // [M + 1]                    the FFT writes bufb
  double* ring = reinterpret_cast<double*>(roots + M + 1);  // [wl] running sums, oldest at `head`
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int tl = g.wl - g.shift;
  double* tail = g.tail + row * tl;
  for (int j = tid; j < g.wl; j += kStftThreads) ring[j] = j < tl ? tail[j] : 0.0;
  build_roots(roots, N, tid);
  int head = 0;
  for (int t = 0; t < g.m; ++t) {
    __syncthreads();  // ring and roots ready / previous hop emitted
    const int64_t base = row * g.stride_r + (int64_t)t * g.stride_t;
    for (int k = tid; k < F; k += kStftThreads) {
      const int64_t e = base + (int64_t)k * g.stride_f;
      double re, im;
      if (g.x_is_c128) {
        const double* p = static_cast<const double*>(g.X) + 2 * e;
        re = p[0];
        im = p[1];
      } else {
        const float* p = static_cast<const float*>(g.X) + 2 * e;
        re = (double)p[0];
        im = (double)p[1];
      }
      if (k == 0 || k == M) im = 0.0;  // numpy.fft.irfft ignores them
      spec[k] = {re, im};
    }
    __syncthreads();
    // Z[k] = Xe + i Xo, Xe = (X[k] + conj X[M-k]) / 2, Xo = (X[k] - conj X[M-k]) / 2 * exp(+2 pi i k / N)
    for (int k = tid; k < M; k += kStftThreads) {
      const Cplx xk = spec[k], xc = spec[M - k];
      const Cplx xe = {0.5 * (xk.re + xc.re), 0.5 * (xk.im - xc.im)};
      const Cplx d = {0.5 * (xk.re - xc.re), 0.5 * (xk.im + xc.im)};
      const Cplx w = {roots[k].re, -roots[k].im};
      const Cplx xo = cmul(d, w);
      bufa[k] = {xe.re - xo.im, xe.im + xo.re};
    }
    __syncthreads();
    const Cplx* z = stockham<+1>(bufa, bufb, roots, M, tid);
    const double scale = 1.0 / (double)M;
    for (int n = tid; n < M; n += kStftThreads) {
      const int m = 2 * n;
      if (m < g.wl) {
        int i = head + m;
        if (i >= g.wl) i -= g.wl;
        ring[i] = add_rounded_product(ring[i], z[n].re, scale, g.window[m]);
      }
      if (m + 1 < g.wl) {
        int i = head + m + 1;
        if (i >= g.wl) i -= g.wl;
        ring[i] = add_rounded_product(ring[i], z[n].im, scale, g.window[m + 1]);
      }
    }
    __syncthreads();
    // the oldest hop is complete: head is a multiple of shift and shift divides wl
    for (int j = tid; j < g.shift; j += kStftThreads) {
      const int64_t q = (int64_t)t * g.shift + j - g.skip;
      if (q >= 0) g.out[row * g.n_out + q] = ring[head + j];
      ring[head + j] = 0.0;
    }
    head += g.shift;
    if (head >= g.wl) head -= g.wl;
  }
  __syncthreads();
  for (int j = tid; j < tl; j += kStftThreads) {
    int i = head + j;
    if (i >= g.wl) i -= g.wl;
    tail[j] = ring[i];
  }
}

}  // namespace

int launch_stft_stream(const StftStreamArgs& a, size_t lds_limit, hipStream_t s) {
  if (!pow2(a.size) || a.size > 8192 || a.wl < 1 || a.wl > a.size || a.shift < 1 || a.m < 0 ||
      a.C < 1 || a.C > 65535 || a.layout < 0 || a.layout > 1)
    return PBBSS_ERR_UNSUPPORTED;
  const int M = a.size / 2;
  const size_t lds = ((size_t)2 * M + M + 1) * sizeof(Cplx);
  if (lds > lds_limit) return PBBSS_ERR_LDS_CAPACITY;
  if (!raise_lds_attribute(stft_stream_kernel, lds)) return PBBSS_ERR_HIP;
  StftStreamArgs g = a;
  if (g.n == 0) {  // nothing of the block is used; the clamped loads still need an address
    g.x = g.hist_in;
    g.x_is_f64 = 1;
  }
  const int groups = g.m > 0 ? (g.m + kFramesPerWg - 1) / kFramesPerWg : 1;
  const dim3 grid((unsigned)groups, (unsigned)g.C);
  hipLaunchKernelGGL(stft_stream_kernel, grid, dim3(kStftThreads), lds, s, g);
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

int launch_istft_stream(const IstftStreamArgs& a, size_t lds_limit, hipStream_t s) {
  if (!pow2(a.size) || a.size > 8192 || a.wl < 1 || a.wl > a.size || a.shift < 1 || a.m < 1 ||
      a.rows < 1 || a.rows > 65535)
    return PBBSS_ERR_UNSUPPORTED;
  const int M = a.size / 2;
  const size_t lds = ((size_t)2 * M + 1 + M + 1) * sizeof(Cplx) + (size_t)a.wl * sizeof(double);
  if (lds > lds_limit) return PBBSS_ERR_LDS_CAPACITY;
  if (!raise_lds_attribute(istft_stream_kernel, lds)) return PBBSS_ERR_HIP;
  hipLaunchKernelGGL(istft_stream_kernel, dim3((unsigned)a.rows), dim3(kStftThreads), lds, s, a);
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

}  // namespace pbbss
