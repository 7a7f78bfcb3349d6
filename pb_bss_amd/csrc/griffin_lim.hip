// Griffin-Lim and MISI phase reconstruction (pb_bss/transform/griffin_lim_module.py:61-64,
// 106-130): given the magnitudes |X| of K sources, iterate
//     X'' = stft(x),   X' = |X| exp(i angle X''),   x_hat = istft(X')
// (MISI: x = x_hat + (y - sum_k x_hat_k) / K in front, equations 4 and 5 of Gunawan & Sen).
//
// One iteration is two ordinary launches:
//   * gl_project_kernel: one 256-thread workgroup takes kFramesPerWg consecutive frames of one
//     signal through window, forward real FFT, magnitude projection, inverse real FFT and
//     synthesis window without leaving LDS (the Stockham FFT of fft_dev.hpp, the packing and
//     untangling of stft.hip), and writes the windowed frames to scratch;
//   * gl_ola_kernel: thread = output sample, the frames covering it added in ascending order;
//     for MISI the same thread owns the sample of all K sources of its mixture and also writes
//     the corrected rows the next projection reads.
// Nothing waits across workgroups; results do not depend on scheduling.  Float64 arithmetic.
#include "griffin_lim.hpp"
#include "fft_dev.hpp"
#include "launch_util.hpp"
#include <cmath>

namespace pbbss {
namespace {

struct ProjectArgs {
  const double* x;        // (S, n) time signals, S = B K
  const void* X;          // (S, T, F) complex64 / complex128
  int x_is_c128;
  int T, size, shift, fade;
  int64_t n;
  const double* awin;     // (size) analysis window
  const double* swin;     // (size) synthesis window
  double* frames;         // (S, T, size)
  double* Xdd;            // (S, T, F) complex128 as (re, im) pairs, or nullptr
  double* Xd;
};

__global__ void __launch_bounds__(kStftThreads) gl_project_kernel(ProjectArgs g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int N = g.size, M = N / 2, F = M + 1;
  Cplx* bufa = reinterpret_cast<Cplx*>(smem);
  Cplx* bufb = bufa + M;
  Cplx* roots = bufb + M;  // [M + 1]
  Cplx* spec = roots + F;  // [F] the projected spectrum X'
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.y;
  const double* xp = g.x + c * g.n;
  build_roots(roots, N, tid);
  for (int ft = 0; ft < kFramesPerWg; ++ft) {
    const int t = blockIdx.x * kFramesPerWg + ft;
    if (t >= g.T) break;  // uniform
    __syncthreads();      // roots ready / previous frame fully written out
    const int64_t s0 = (int64_t)t * g.shift - g.fade;
    for (int n = tid; n < M; n += kStftThreads) {
      // loads at clamped indices, masks afterwards (as stft_kernel)
      double v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int m = 2 * n + h;
        const int64_t si = s0 + m;
        const bool ok = si >= 0 && si < g.n;
        const double xv = xp[ok ? si : 0];
        v[h] = ok ? xv * g.awin[m] : 0.0;
      }
      bufa[n] = {v[0], v[1]};
    }
    __syncthreads();
    const Cplx* Z = stockham<-1>(bufa, bufb, roots, M, tid);
    const size_t base = ((size_t)c * g.T + t) * F;
    // untangle (stft_kernel), then keep the phase of X'' and take the magnitude of X
    for (int k = tid; k < F; k += kStftThreads) {
      const Cplx zk = Z[k & (M - 1)], zc = Z[(M - k) & (M - 1)];
      const Cplx xe = {0.5 * (zk.re + zc.re), 0.5 * (zk.im - zc.im)};
      const Cplx xo = {0.5 * (zk.im + zc.im), -0.5 * (zk.re - zc.re)};
      const Cplx r = cmul(roots[k], xo);
      const double dre = xe.re + r.re, dim = xe.im + r.im;
      double mre, mim;
      if (g.x_is_c128) {
        const double* p = static_cast<const double*>(g.X) + 2 * (base + k);
        mre = p[0];
        mim = p[1];
      } else {
        const float* p = static_cast<const float*>(g.X) + 2 * (base + k);
        mre = (double)p[0];
        mim = (double)p[1];
      }
      const double mag = hypot(mre, mim);
      const double len = hypot(dre, dim);
      // angle(0) = 0: the phase factor of an exactly zero bin is 1
      const Cplx out = len == 0.0 ? Cplx{mag, 0.0} : Cplx{mag * (dre / len), mag * (dim / len)};
      if (g.Xdd) {
        g.Xdd[2 * (base + k)] = dre;
        g.Xdd[2 * (base + k) + 1] = dim;
        g.Xd[2 * (base + k)] = out.re;
        g.Xd[2 * (base + k) + 1] = out.im;
      }
      // numpy.fft.irfft ignores the imaginary parts of bins 0 and N/2
      spec[k] = {out.re, (k == 0 || k == M) ? 0.0 : out.im};
    }
    __syncthreads();
    // pack for the inverse (istft_frames_kernel): Z[k] = Xe + i Xo
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
    double* o = g.frames + ((size_t)c * g.T + t) * N;
    for (int n = tid; n < M; n += kStftThreads) {
      const int m = 2 * n;
      o[m] = z[n].re * scale * g.swin[m];
      o[m + 1] = z[n].im * scale * g.swin[m + 1];
    }
  }
}

struct OlaArgs {
  const double* frames;  // (B, K, T, size); nullptr: the sums are the rows of x_hat (first guess)
  const double* y;       // (B, n) mixtures: MISI; nullptr: Griffin-Lim
  int K, T, size, shift, fade;
  int64_t n;
  double* x_hat;         // (B, K, n); written unless frames is nullptr
  double* next;          // (B, K, n) x_hat + (y - sum_k x_hat_k) / K, or nullptr
};

// thread = output sample n of the K rows of mixture blockIdx.y; KMAX = 1: of row blockIdx.y
template <int KMAX>
__global__ void __launch_bounds__(kStftThreads) gl_ola_kernel(OlaArgs g) {
  const int64_t n = (int64_t)blockIdx.x * kStftThreads + threadIdx.x;
  if (n >= g.n) return;
  const int K = KMAX == 1 ? 1 : g.K;
  const int64_t row0 = (int64_t)blockIdx.y * K;
  const int64_t m = n + g.fade;
  int64_t t_hi = m / g.shift;
  if (t_hi > g.T - 1) t_hi = g.T - 1;
  int64_t t_lo = (m - g.size + g.shift) / g.shift;  // ceil((m - size + 1) / shift)
  if (m - g.size + 1 <= 0) t_lo = 0;
  double acc[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k >= K) break;
    const int64_t row = row0 + k;
    if (g.frames) {
      double a = 0.0;
      for (int64_t t = t_lo; t <= t_hi; ++t)
        a += g.frames[((size_t)row * g.T + t) * g.size + (m - t * g.shift)];
      acc[k] = a;
      g.x_hat[row * g.n + n] = a;
    } else {
      acc[k] = g.x_hat[row * g.n + n];
    }
  }
  if (!g.next) return;
  double sum = acc[0];  // k ascending, as numpy.sum(axis=0)
#pragma unroll
  for (int k = 1; k < KMAX; ++k)
    if (k < K) sum += acc[k];
  const double e = (g.y[(int64_t)blockIdx.y * g.n + n] - sum) / (double)K;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) g.next[(row0 + k) * g.n + n] = acc[k] + e;
}

}  // namespace

size_t griffin_lim_scratch_bytes(const GriffinLimProblem& p) {
  const size_t S = (size_t)p.B * p.K;
  return (S * p.T * p.size + (p.y ? S * (size_t)p.n : 0)) * sizeof(double);
}

int run_griffin_lim(const GriffinLimProblem& p, void* scratch, size_t lds_limit, hipStream_t s) {
  const int64_t S = p.B * p.K;
  if (!pow2(p.size) || p.size > 8192 || p.shift < 1 || p.size % p.shift || p.T < 1 || p.K < 1 ||
      p.B < 1 || S > 65535 || p.n < 1 || p.iterations < 0)
    return PBBSS_ERR_UNSUPPORTED;
  if (p.y && p.K > kMisiMaxSources) return PBBSS_ERR_UNSUPPORTED;
  const int M = p.size / 2;
  const size_t lds = ((size_t)2 * M + 2 * (M + 1)) * sizeof(Cplx);
  if (lds > lds_limit) return PBBSS_ERR_LDS_CAPACITY;
  if (!raise_lds_attribute(gl_project_kernel, lds)) return PBBSS_ERR_HIP;

  double* frames = static_cast<double*>(scratch);
  double* corrected = p.y ? frames + (size_t)S * p.T * p.size : nullptr;
  const dim3 block(kStftThreads);
  const dim3 grid_project((unsigned)((p.T + kFramesPerWg - 1) / kFramesPerWg), (unsigned)S);
  const unsigned span = (unsigned)((p.n + kStftThreads - 1) / kStftThreads);
  OlaArgs o{frames, p.y, p.K, p.T, p.size, p.shift, p.fade, p.n, p.x_hat, corrected};
  auto overlap_add = [&](const OlaArgs& a) {
    if (p.y)
      hipLaunchKernelGGL(gl_ola_kernel<kMisiMaxSources>, dim3(span, (unsigned)p.B), block, 0, s, a);
    else
      hipLaunchKernelGGL(gl_ola_kernel<1>, dim3(span, (unsigned)S), block, 0, s, a);
  };
  if (p.y && p.iterations > 0) {  // the correction of the first guess (MISI.step does it first)
    OlaArgs first = o;
    first.frames = nullptr;
    overlap_add(first);
  }
  for (int it = 0; it < p.iterations; ++it) {
    const bool last = it == p.iterations - 1;
    ProjectArgs g{p.y ? corrected : p.x_hat, p.X, p.x_is_c128, p.T, p.size, p.shift, p.fade, p.n,
                  p.analysis_window, p.synthesis_window, frames,
                  last ? static_cast<double*>(p.X_dash_dash) : nullptr,
                  last ? static_cast<double*>(p.X_dash) : nullptr};
    hipLaunchKernelGGL(gl_project_kernel, grid_project, block, lds, s, g);
    if (last) o.next = nullptr;  // nothing reads the corrected rows after the last iteration
    overlap_add(o);
  }
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

}  // namespace pbbss
