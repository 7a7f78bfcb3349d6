// In-LDS radix-2 Stockham FFT shared by the STFT kernels (stft.hip) and the Griffin-Lim
// projection (griffin_lim.hip): one 256-thread workgroup, float64, a table of N-th roots of
// unity that serves both the FFT stages (M-th roots = every second entry, M = N/2) and the
// untangling of a real transform packed into M complex points.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace pbbss {
namespace {

constexpr int kStftThreads = 256;
constexpr int kFramesPerWg = 4;

struct Cplx {
  double re, im;
};

__device__ __forceinline__ Cplx cmul(Cplx a, Cplx b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

// roots[k] = exp(-2 pi i k / N), k = 0..M (M = N/2)
__device__ void build_roots(Cplx* roots, int N, int tid) {
  const int M = N / 2;
  for (int k = tid; k <= M; k += kStftThreads) {
    double s, c;
    sincospi(-2.0 * (double)k / (double)N, &s, &c);
    roots[k] = {c, s};
  }
}

// In-LDS radix-2 Stockham FFT of M points (M a power of two >= 2).  SIGN = -1 forward,
// +1 backward (unscaled).  Returns the buffer that holds the result.
template <int SIGN>
__device__ Cplx* stockham(Cplx* a, Cplx* b, const Cplx* roots, int M, int tid) {
  int n = M, s = 1, ls = 0;  // s = 2^ls butterflies share a twiddle
  while (n > 1) {
    const int half = n >> 1;
    for (int j = tid; j < (M >> 1); j += kStftThreads) {
      const int p = j >> ls, q = j & (s - 1);
      Cplx w = roots[2 * (p << ls)];  // exp(-2 pi i p / n) = roots_N[2 p M / n]
      if (SIGN > 0) w.im = -w.im;
      const Cplx u = a[q + s * p], v = a[q + s * (p + half)];
      b[q + s * (2 * p)] = {u.re + v.re, u.im + v.im};
      b[q + s * (2 * p + 1)] = cmul({u.re - v.re, u.im - v.im}, w);
    }
    __syncthreads();
    Cplx* t = a;
    a = b;
    b = t;
    n = half;
    s <<= 1;
    ++ls;
  }
  return a;
}

inline bool pow2(int v) { return v >= 4 && (v & (v - 1)) == 0; }

}  // namespace
}  // namespace pbbss
