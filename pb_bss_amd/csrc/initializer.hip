// Deflation seed (pb_bss/initializer/deflation.py:6-89) on the device.
//
// One workgroup of 256 threads per (utterance, bin).  A deflation round of a bin is
//   peak frame   arg-max of the saliency row (per-bin form) or of the mean saliency over all
//                bins of the utterance (permutation-free form, read from device memory),
//                lowest index among ties, clipped to [neighbors, T - 1 - neighbors];
//   local PSD    over the 2 neighbors + 1 frames around it, the local saliencies as the mask,
//                normalised by max(sum, 1e-10) (extraction/beamformer.py:127-139);
//   mode         eigenvector of its largest eigenvalue (get_pca_vector, beamformer.py:163-224):
//                wave 0 runs the cyclic Jacobi of wave_la.hpp on the D x D matrix, lane (i, j)
//                owning entry (i, j);
//   similarity   |z_t^H mode|^2 with z_t = y_t / max(|y_t|, tiny)
//                (permutation_alignment.py:358-377) -- the posterior of the round's class;
//   deflation    saliency_t *= 1 - similarity_t.
// After K - 1 rounds the last class takes 1 - sum, everything is floored at eps and normalised
// over the classes.
//
// Per-bin form, 2 <= D <= 8: all rounds of a bin in ONE launch, the bin's frames and its
// saliency row resident in LDS (dynamic LDS: T doubles, then T * D complex values of the input
// type).  Frames that do not fit stay where they are -- the observation is only read, so the
// "slab" of a long utterance is the input itself -- and a saliency row that does not fit lives in
// the (B, F, T) state array; the code is the same, through generic pointers.
//
// Permutation-free form: the peak frame needs the saliencies of every bin of the utterance.
// That cross-bin step is a launch boundary, never a wait inside a kernel:
//   init (saliency rows -> state) | column mean | round 0 | column mean | round 1 | ...
// i.e. 2 (K - 1) + 1 stream-ordered launches.  The column mean (B, T) stays in device memory and
// every bin's workgroup takes the arg-max of it itself (T values from L2), so no index ever
// travels through the host and the call can be captured into a HIP graph.  Here the rows are
// used where they lie (each value is touched once per launch: staging would only add a copy).
//
// 9 <= D <= 32: the round is split at the eigenproblem -- PSD to memory, the generic
// launch_gen_heev (generic.hip), similarity and deflation -- three launches per round.
#include "initializer.hpp"
#include <limits>
#include "generic.hpp"
#include "launch_util.hpp"
#include "pbbss.h"
#include "pbbss_dev.hpp"
#include "wave_la.hpp"

namespace pbbss {
namespace {

constexpr int kDsThreads = 256;
constexpr int kDsWaves = kDsThreads / kWave;
constexpr int kDsMaxD = 32;
constexpr size_t kDsStaticLds = 2048;  // static LDS of the bin kernel, rounded up
enum { kPhasePre = 1, kPhasePost = 2, kPhaseAll = 3 };

template <typename Y2>
__device__ __forceinline__ void widen(const Y2 v, double& re, double& im) {
  re = (double)v.x;
  im = (double)v.y;
}

// does candidate (av, ai) precede (bv, bi) as the arg-max?  np.argmax: the first NaN wins, else
// the larger value, else the lower index.
__device__ __forceinline__ bool peak_before(double av, int ai, double bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return an && (!bn || ai < bi);
  return av > bv || (av == bv && ai < bi);
}

// arg-max of v[0 .. T) over the workgroup; every thread calls, every thread gets the index
__device__ __forceinline__ int block_argmax(const double* v, int T, int tid, double* red_v,
                                            int* red_i) {
  double bv = -std::numeric_limits<double>::infinity();
  int bi = T;
  for (int t = tid; t < T; t += kDsThreads) {
    const double x = v[t];
    if (peak_before(x, t, bv, bi)) {
      bv = x;
      bi = t;
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double ov = __shfl_xor(bv, off, kWave);
    const int oi = __shfl_xor(bi, off, kWave);
    if (peak_before(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  __syncthreads();  // red_* of the previous round have been read
  if ((tid & (kWave - 1)) == 0) {
    red_v[tid / kWave] = bv;
    red_i[tid / kWave] = bi;
  }
  __syncthreads();
  bv = red_v[0];
  bi = red_i[0];
#pragma unroll
  for (int w = 1; w < kDsWaves; ++w)
    if (peak_before(red_v[w], red_i[w], bv, bi)) {
      bv = red_v[w];
      bi = red_i[w];
    }
  return bi;
}

// DT: compile-time sensor count of the fused kernel (2..8), 0: run-time D, eigenproblem outside
template <int DT, typename Y2>
__global__ __launch_bounds__(kDsThreads) void deflation_bin_kernel(DeflationArgs a, int init,
                                                                   int phase, int lds_sal,
                                                                   int lds_y) {
  extern __shared__ double ds_lds[];
  __shared__ double red_v[kDsWaves];
  __shared__ int red_i[kDsWaves];
  __shared__ double mode[2 * kDsMaxD];
  const int tid = threadIdx.x;
  const int64_t n = blockIdx.x;  // bin: b * F + f
  const int64_t b = n / a.F;
  const int f = (int)(n - b * a.F);
  const int T = a.T, K = a.K, nb = a.neighbors;
  const int D = DT > 0 ? DT : a.D;
  const Y2* yp = static_cast<const Y2*>(a.y) + n * T * D;
  double* sal = lds_sal ? ds_lds : a.sal_state + n * T;
  double* outb = a.out + (b * K * a.F + f) * (int64_t)T;  // class k at + k * F * T
  const int64_t kstride = (int64_t)a.F * T;

  if (lds_y) {
    Y2* yl = reinterpret_cast<Y2*>(ds_lds + (lds_sal ? T : 0));
    for (int i = tid; i < T * D; i += kDsThreads) yl[i] = yp[i];
    yp = yl;
    __syncthreads();
  }
  if (init) {
    for (int t = tid; t < T; t += kDsThreads) {
      double s;
      if (a.sal_in) {
        s = a.sal_in[n * T + t];
      } else {
        double n2 = 0.0;
        for (int d = 0; d < D; ++d) {
          double re, im;
          widen(yp[t * D + d], re, im);
          n2 += re * re + im * im;
        }
        s = sqrt(n2);
      }
      sal[t] = s;
    }
  }
  __syncthreads();

  for (int r = a.r0; r < a.r1; ++r) {
    if (phase & kPhasePre) {
      const double* src = a.permutation_free ? a.colmean + b * T : sal;
      int peak = block_argmax(src, T, tid, red_v, red_i);
      peak = min(max(peak, nb), T - 1 - nb);
      if (a.out_peak && tid == 0) a.out_peak[(b * (K - 1) + r) * a.F + f] = peak;
      const int t0 = peak - nb, L = 2 * nb + 1;
      if constexpr (DT > 0) {
        if (tid < kWave) {
          const LaneIJ c = lane_ij(tid);
          double den = 0.0;
          for (int l = 0; l < L; ++l) den += sal[t0 + l];
          den = fmax(den, 1e-10);
          double are = 0.0, aim = 0.0;
          if (c.i < D && c.j < D) {
            for (int l = 0; l < L; ++l) {
              const double w = sal[t0 + l] / den;
              double ir, ii, jr, ji;
              widen(yp[(t0 + l) * D + c.i], ir, ii);
              widen(yp[(t0 + l) * D + c.j], jr, ji);
              are += w * (ir * jr + ii * ji);
              aim += w * (ii * jr - ir * ji);
            }
          }
          double vre, vim;
          (void)wave_jacobi_heev<DT>(are, aim, c, vre, vim);
          const bool col = c.j < D;
          const double lam = lane_get(are, ij_lane(col ? c.j : 0, col ? c.j : 0));
          const double top = wave_max(col ? lam : -std::numeric_limits<double>::infinity());
          const int jbest = (int)-wave_max((col && lam == top) ? -(double)c.j : -99.0);
          // a non-finite PSD has no largest eigenvalue: the whole bin becomes NaN, as it does
          // in the reference
          const bool bad = jbest >= D;
          if (c.i < D && c.j == (bad ? 0 : jbest)) {
            const double nan = std::numeric_limits<double>::quiet_NaN();
            mode[2 * c.i] = bad ? nan : vre;
            mode[2 * c.i + 1] = bad ? nan : vim;
          }
        }
      } else {
        double den = 0.0;
        for (int l = 0; l < L; ++l) den += sal[t0 + l];
        den = fmax(den, 1e-10);
        double* psd = a.psd + n * D * D * 2;
        for (int e = tid; e < D * D; e += kDsThreads) {
          const int i = e / D, j = e - i * D;
          double are = 0.0, aim = 0.0;
          for (int l = 0; l < L; ++l) {
            const double w = sal[t0 + l] / den;
            double ir, ii, jr, ji;
            widen(yp[(t0 + l) * D + i], ir, ii);
            widen(yp[(t0 + l) * D + j], jr, ji);
            are += w * (ir * jr + ii * ji);
            aim += w * (ii * jr - ir * ji);
          }
          psd[2 * e] = are;
          psd[2 * e + 1] = (i == j) ? 0.0 : aim;
        }
      }
    }
    if (!(phase & kPhasePost)) continue;
    if constexpr (DT == 0) {
      // eigenvalues ascending, eigenvectors in columns: the mode is the last column
      const double* vec = a.eigvec + n * D * D * 2;
      if (tid < D) {
        mode[2 * tid] = vec[(tid * D + D - 1) * 2];
        mode[2 * tid + 1] = vec[(tid * D + D - 1) * 2 + 1];
      }
    }
    __syncthreads();
    {  // mode / max(|mode|, tiny)
      double m2 = 0.0;
      for (int d = 0; d < D; ++d) m2 += mode[2 * d] * mode[2 * d] + mode[2 * d + 1] * mode[2 * d + 1];
      const double den = fmax(sqrt(m2), kTiny);
      __syncthreads();
      if (tid < 2 * D) mode[tid] = (m2 != m2) ? m2 : mode[tid] / den;
      __syncthreads();
    }
    double* outk = outb + r * kstride;
    for (int t = tid; t < T; t += kDsThreads) {
      double pr = 0.0, pi = 0.0, n2 = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        double yr, yi;
        widen(yp[t * D + d], yr, yi);
        const double mr = mode[2 * d], mi = mode[2 * d + 1];
        n2 += yr * yr + yi * yi;
        pr += yr * mr + yi * mi;  // conj(y) m
        pi += yr * mi - yi * mr;
      }
      const double den = fmax(sqrt(n2), kTiny);
      pr /= den;
      pi /= den;
      const double sim = pr * pr + pi * pi;
      outk[t] = sim;
      sal[t] = sal[t] * (1.0 - sim);
    }
    __syncthreads();
  }

  if (a.finalize) {
    const double eps = a.eps;
    for (int t = tid; t < T; t += kDsThreads) {
      double s = 0.0;
      for (int k = 0; k < K - 1; ++k) s += outb[k * kstride + t];
      double last = 1.0 - s;
      last = (last < eps) ? eps : last;  // a select keeps a NaN, as np.maximum does
      double tot = 0.0;
      for (int k = 0; k < K - 1; ++k) {
        double p = outb[k * kstride + t];
        p = (p < eps) ? eps : p;
        tot += p;
      }
      tot += last;
      for (int k = 0; k < K - 1; ++k) {
        double p = outb[k * kstride + t];
        p = (p < eps) ? eps : p;
        outb[k * kstride + t] = p / tot;
      }
      outb[(K - 1) * kstride + t] = last / tot;
    }
  }
}

// colmean[b, t] = mean over the F bins of state[b, :, t]; four partial sums over contiguous
// bin ranges, combined in a fixed order (the result does not depend on the batch or the launch)
__global__ __launch_bounds__(kDsThreads) void deflation_colmean_kernel(const double* state, int F,
                                                                       int T, double* colmean) {
  __shared__ double part[kDsWaves][kWave];
  const int lane = threadIdx.x & (kWave - 1), g = threadIdx.x / kWave;
  const int t = blockIdx.x * kWave + lane;
  const int64_t b = blockIdx.y;
  const int per = (F + kDsWaves - 1) / kDsWaves;
  const int f0 = g * per, f1 = min(F, f0 + per);
  double s = 0.0;
  if (t < T) {
    const double* p = state + (b * F + f0) * (int64_t)T + t;
#pragma unroll 8
    for (int f = f0; f < f1; ++f, p += T) s += *p;
  }
  part[g][lane] = s;
  __syncthreads();
  if (g == 0 && t < T)
    colmean[b * T + t] = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) / F;
}

inline int ds_ok() { return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP; }

struct DsPlan {
  bool fused, single, lds_sal, lds_y, need_state;
  size_t lds;
};

DsPlan ds_plan(const DeflationArgs& a, int init, size_t lds_limit) {
  DsPlan p{};
  p.fused = a.D <= 8;
  // every round of a bin in one launch: per-bin peaks, in-kernel eigenproblem
  p.single = p.fused && !a.permutation_free;
  const size_t budget = lds_limit > kDsStaticLds ? lds_limit - kDsStaticLds : 0;
  const size_t sal_b = (size_t)a.T * sizeof(double);
  const size_t y_b = (size_t)a.T * a.D * (a.y_is_c128 ? 16 : 8);
  const bool whole = p.single && init && a.finalize && a.r1 == a.K - 1;
  p.lds_sal = whole && sal_b <= budget;
  p.lds_y = p.single && a.r1 > a.r0 && (p.lds_sal ? sal_b : 0) + y_b <= budget;
  p.need_state = !p.lds_sal;
  p.lds = (p.lds_sal ? sal_b : 0) + (p.lds_y ? y_b : 0);
  return p;
}

template <int DT, typename Y2>
int launch_bin(const DeflationArgs& a, int init, int phase, bool lds_sal, bool lds_y, size_t lds,
               hipStream_t s) {
  auto kfn = deflation_bin_kernel<DT, Y2>;
  if (lds > 0 && !raise_lds_attribute(kfn, lds)) return PBBSS_ERR_HIP;
  hipLaunchKernelGGL(kfn, dim3((unsigned)(a.B * a.F)), dim3(kDsThreads), lds, s, a, init, phase,
                     (int)lds_sal, (int)lds_y);
  return ds_ok();
}

template <typename Y2>
int launch_bin_d(const DeflationArgs& a, int init, int phase, bool lds_sal, bool lds_y, size_t lds,
                 hipStream_t s) {
  switch (a.D) {
    case 2: return launch_bin<2, Y2>(a, init, phase, lds_sal, lds_y, lds, s);
    case 3: return launch_bin<3, Y2>(a, init, phase, lds_sal, lds_y, lds, s);
    case 4: return launch_bin<4, Y2>(a, init, phase, lds_sal, lds_y, lds, s);
    case 5: return launch_bin<5, Y2>(a, init, phase, lds_sal, lds_y, lds, s);
    case 6: return launch_bin<6, Y2>(a, init, phase, lds_sal, lds_y, lds, s);
    case 7: return launch_bin<7, Y2>(a, init, phase, lds_sal, lds_y, lds, s);
    case 8: return launch_bin<8, Y2>(a, init, phase, lds_sal, lds_y, lds, s);
    default: return launch_bin<0, Y2>(a, init, phase, lds_sal, lds_y, lds, s);
  }
}

int launch_bin_any(const DeflationArgs& a, int init, int phase, bool lds_sal, bool lds_y,
                   size_t lds, hipStream_t s) {
  return a.y_is_c128 ? launch_bin_d<double2>(a, init, phase, lds_sal, lds_y, lds, s)
                     : launch_bin_d<float2>(a, init, phase, lds_sal, lds_y, lds, s);
}

size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

size_t deflation_work_bytes(const DeflationArgs& a, int init, size_t lds_limit) {
  const DsPlan p = ds_plan(a, init, lds_limit);
  const size_t N = (size_t)a.B * a.F, D = (size_t)a.D;
  size_t bytes = 0;
  if (p.need_state && !a.sal_state) bytes += pad256(N * a.T * sizeof(double));
  if (a.permutation_free) bytes += pad256((size_t)a.B * a.T * sizeof(double));
  if (!p.fused)
    bytes += 2 * pad256(N * D * D * 2 * sizeof(double)) + pad256(N * D * sizeof(double)) +
             pad256(N * sizeof(int32_t));
  return bytes;
}

int launch_deflation_seed(DeflationArgs a, int init, void* work, size_t lds_limit, hipStream_t s) {
  if (a.D < 2 || a.D > kDsMaxD || a.K < 2 || a.K > 19) return PBBSS_ERR_UNSUPPORTED;
  if (a.B <= 0 || a.F <= 0 || a.T <= 0 || a.neighbors < 0 || a.T <= 2 * a.neighbors ||
      a.r0 < 0 || a.r1 < a.r0 || a.r1 > a.K - 1)
    return PBBSS_ERR_INVALID_ARG;
  if (a.B > 65535 || a.B * a.F > 0x7fffffff) return PBBSS_ERR_UNSUPPORTED;
  const DsPlan p = ds_plan(a, init, lds_limit);
  const size_t N = (size_t)a.B * a.F, D = (size_t)a.D;
  char* w = static_cast<char*>(work);
  auto take = [&](size_t bytes) {
    char* r = w;
    w += pad256(bytes);
    return r;
  };
  if (p.need_state && !a.sal_state) a.sal_state = reinterpret_cast<double*>(take(N * a.T * sizeof(double)));
  if (a.permutation_free) a.colmean = reinterpret_cast<double*>(take((size_t)a.B * a.T * sizeof(double)));
  if (!p.fused) {
    a.psd = reinterpret_cast<double*>(take(N * D * D * 2 * sizeof(double)));
    a.eigvec = reinterpret_cast<double*>(take(N * D * D * 2 * sizeof(double)));
    a.eigval = reinterpret_cast<double*>(take(N * D * sizeof(double)));
    a.eigst = reinterpret_cast<int32_t*>(take(N * sizeof(int32_t)));
  }

  if (p.single) return launch_bin_any(a, init, kPhaseAll, p.lds_sal, p.lds_y, p.lds, s);

  const int r0 = a.r0, r1 = a.r1, fin = a.finalize;
  int rc;
  if (init) {  // saliency rows -> state
    a.r1 = r0;
    a.finalize = 0;
    if ((rc = launch_bin_any(a, 1, kPhaseAll, false, false, 0, s)) != PBBSS_OK) return rc;
  }
  for (int r = r0; r < r1; ++r) {
    a.r0 = r;
    a.r1 = r + 1;
    a.finalize = fin && r == r1 - 1;
    if (a.permutation_free) {
      hipLaunchKernelGGL(deflation_colmean_kernel, dim3((unsigned)((a.T + kWave - 1) / kWave), (unsigned)a.B),
                         dim3(kDsThreads), 0, s, a.sal_state, a.F, a.T, a.colmean);
      if ((rc = ds_ok()) != PBBSS_OK) return rc;
    }
    if (p.fused) {
      if ((rc = launch_bin_any(a, 0, kPhaseAll, false, false, 0, s)) != PBBSS_OK) return rc;
    } else {
      const int f2 = a.finalize;
      a.finalize = 0;
      if ((rc = launch_bin_any(a, 0, kPhasePre, false, false, 0, s)) != PBBSS_OK) return rc;
      if ((rc = launch_gen_heev(a.psd, (int64_t)N, a.D, -1, 0.0, a.eigval, a.eigvec, a.eigst,
                                lds_limit, s)) != PBBSS_OK)
        return rc;
      a.finalize = f2;
      if ((rc = launch_bin_any(a, 0, kPhasePost, false, false, 0, s)) != PBBSS_OK) return rc;
    }
  }
  if (fin && r0 == r1) {
    a.r0 = a.r1 = r0;
    a.finalize = 1;
    if ((rc = launch_bin_any(a, 0, kPhaseAll, false, false, 0, s)) != PBBSS_OK) return rc;
  }
  return PBBSS_OK;
}

}  // namespace pbbss
