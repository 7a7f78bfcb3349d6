// Device helpers shared by the evaluation kernels (eval.hip, bss_eval.hip): ordered sums and the
// search over selections in itertools.permutations order.
#pragma once
#include "eval.hpp"

namespace pbbss {

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// sum of the `chunks` partials of one accumulator, in span order
__device__ inline double span_sum(const double* p, int64_t chunks, int64_t stride) {
  double s = p[0];
  for (int64_t w = 1; w < chunks; ++w) s += p[w * stride];
  return s;
}

// NumPy's summation order for a short run of float64 (add.reduce along a contiguous axis):
// fewer than 8 addends one after the other from zero, otherwise eight running sums over the
// blocks of eight, combined as a tree, and the remainder one after the other.
__device__ inline double np_sum(const double* a, int n, int stride) {
  if (n < 8) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += a[i * stride];
    return s;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = a[j * stride];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += a[(i + j) * stride];
  }
  double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) s += a[i * stride];
  return s;
}

// selection number p (itertools.permutations(range(Kt), Ks) order) -> sel[0..Ks)
__device__ inline void unrank_selection(int p, int Ks, int Kt, const int (&radix)[kSxrMaxTargets],
                                        int (&sel)[kSxrMaxTargets]) {
  unsigned used = 0;
#pragma unroll
  for (int k = 0; k < kSxrMaxTargets; ++k) {
    sel[k] = 0;
    if (k < Ks) {
      int d = p / radix[k];
      p -= d * radix[k];
      int pick = 0;
      bool found = false;
#pragma unroll
      for (int t = 0; t < kSxrMaxTargets; ++t) {
        const bool is_free = t < Kt && !((used >> t) & 1u);
        if (is_free && !found) {
          if (d == 0) {
            pick = t;
            found = true;
          }
          --d;
        }
      }
      sel[k] = pick;
      used |= 1u << pick;
    }
  }
}

// is candidate (va, pa) ahead of (vb, pb) for np.argmax: larger value, NaN ahead of everything,
// lower index among equals
__device__ inline bool ahead(double va, int pa, double vb, int pb) {
  const bool na = va != va, nb = vb != vb;
  if (na != nb) return na;
  if (!na && va != vb) return va > vb;
  return pa < pb;
}

}  // namespace pbbss
