// Complex circular-symmetric Gaussian of a sensor vector (include/pbbss.h, XII; reference
// distribution/complex_circular_symmetric_gaussian.py): the saliency-weighted covariance of
// `_fit` and the log-pdf, on frames in the reference's own (B, N, D) layout.
//
// Both kernels stage the frames of one workgroup -- ccsg_frames(D) consecutive rows of y, which
// are one contiguous piece of memory -- through LDS with 16-byte loads, widened to complex128,
// each row padded to an odd number of 16-byte slots (a lane that walks its own row then meets
// no bank conflict with its neighbours).
//
// fit:     one workgroup per (batch item, span of frames).  A thread owns one entry of the lower
//          triangle (or the saliency sums) for all classes of a class tile -- the product
//          y_d conj(y_e) of a frame is formed once and weighted K times -- and, where the entries
//          are fewer than the threads, one interleaved slice of the span; slices are added in
//          ascending order.  Every workgroup writes its partial sums; a second kernel adds the
//          spans in ascending order, divides and mirrors.  No atomics: the result does not depend
//          on scheduling.
// log_pdf: one launch.  A workgroup takes a tile of frames of one batch item and all classes, a
//          class tile at a time: the lower triangles go to LDS, one wavefront per matrix factors
//          it (left-looking Cholesky, lane = row), then lane = frame solves L z = y by forward
//          substitution with z in registers (loops unrolled for the instantiation's D bound) and
//          L read from LDS by broadcast; the quadratic form is the sum of |z_j|^2.
#include "ccsg.hpp"
#include <math.h>
#include "launch_util.hpp"

namespace pbbss {
namespace {

constexpr int kFitThreads = 256;

__device__ __forceinline__ double2 widen(float2 v) { return make_double2((double)v.x, (double)v.y); }

// LDS operations of one wavefront execute in program order; this keeps the compiler from
// reordering them around a hand-over between lanes of the wavefront.
__device__ __forceinline__ void wave_lds_fence() { __asm__ volatile("" ::: "memory"); }

// `cnt` = frames * D consecutive complex elements of y, from element `e0` on, to
// ys[frame * DS + d] as complex128.  16-byte loads: one complex128, or two complex64 from the
// first 16-byte boundary on (an odd element in front and behind goes alone).
template <int NT>
__device__ __forceinline__ void stage_frames(const void* y, int c128, int64_t e0, int cnt, int D,
                                             int DS, double2* ys, int tid) {
  auto put = [&](int e, double2 v) {
    const int n = e / D;
    ys[n * DS + (e - n * D)] = v;
  };
  if (c128) {
    const double2* p = static_cast<const double2*>(y) + e0;
    for (int e = tid; e < cnt; e += NT) put(e, p[e]);
    return;
  }
  const float2* p = static_cast<const float2*>(y) + e0;
  int head = (int)((reinterpret_cast<uintptr_t>(p) >> 3) & 1);
  if (head > cnt) head = cnt;
  const int pairs = (cnt - head) >> 1;
  const float4* q = reinterpret_cast<const float4*>(p + head);
  if (tid == 0 && head) put(0, widen(p[0]));
  for (int i = tid; i < pairs; i += NT) {
    const float4 v = q[i];
    put(head + 2 * i, make_double2((double)v.x, (double)v.y));
    put(head + 2 * i + 1, make_double2((double)v.z, (double)v.w));
  }
  if (tid == 0 && ((cnt - head) & 1)) put(cnt - 1, widen(p[cnt - 1]));
}

// ------------------------------------------------------------------------------------------ fit
// part[((b * spans + span) * K + k) * (tri + 1) + q]: q < tri the entry (d, e <= d) of the lower
// triangle at q = d (d + 1) / 2 + e, q = tri the saliency sum (real part).
template <typename S>
__global__ __launch_bounds__(kFitThreads) void ccsg_fit_kernel(const void* y, int c128, int64_t N,
                                                               int D, int K, int spans,
                                                               const S* sal, double2* part) {
  extern __shared__ double2 ccsg_lds[];
  const int tid = threadIdx.x;
  const int FT = ccsg_frames(D), DS = D | 1;
  const int64_t b = blockIdx.x / spans;
  const int span = (int)(blockIdx.x - b * spans);
  const int64_t n0 = (int64_t)span * FT;
  const int nf = (int)(N - n0 < FT ? N - n0 : FT);
  const int tri = D * (D + 1) / 2, Q = tri + 1;
  const int ka = K < kCcsgMaxClassTile ? K : kCcsgMaxClassTile;  // classes in LDS at a time
  double2* ys = ccsg_lds;
  double* ss = reinterpret_cast<double*>(ys + FT * DS);
  double2* red = reinterpret_cast<double2*>(ss + ka * FT);
  // a thread owns one entry q of the triangle (q = tri: the saliency sums, "y_d conj(y_e)" = 1)
  // for all classes of the tile and, where the entries are fewer than the threads, slice g of G
  // interleaved slices of the span
  const int G = Q < kFitThreads ? kFitThreads / Q : 1;
  stage_frames<kFitThreads>(y, c128, (b * N + n0) * D, nf * D, D, DS, ys, tid);
  for (int k0 = 0; k0 < K; k0 += kCcsgMaxClassTile) {
    const int kt = K - k0 < kCcsgMaxClassTile ? K - k0 : kCcsgMaxClassTile;
    if (k0) __syncthreads();  // the previous class tile has been read
    if (sal)
      for (int e = tid; e < kt * nf; e += kFitThreads) {
        const int kk = e / nf, n = e - kk * nf;
        ss[kk * FT + n] = (double)sal[((b * K + k0 + kk) * N) + n0 + n];
      }
    __syncthreads();  // frames (loaded beside the first saliencies) and saliencies are staged
    double2* out = part + ((b * spans + span) * K + k0) * Q;
    for (int idx = tid; idx < Q * G; idx += kFitThreads) {
      const int g = idx / Q, q = idx - g * Q;
      const bool one = q == tri;
      int d = 0;
      while (!one && (d + 1) * (d + 2) / 2 <= q) ++d;
      const int e = one ? 0 : q - d * (d + 1) / 2;
      double ar[kCcsgMaxClassTile], ai[kCcsgMaxClassTile];
#pragma unroll
      for (int kk = 0; kk < kCcsgMaxClassTile; ++kk) ar[kk] = ai[kk] = 0.0;
#pragma unroll 2
      for (int n = g; n < nf; n += G) {
        const double2 a = ys[n * DS + d], c = ys[n * DS + e];
        const double pr = one ? 1.0 : a.x * c.x + a.y * c.y;  // y_d conj(y_e)
        const double pi = one ? 0.0 : a.y * c.x - a.x * c.y;
#pragma unroll
        for (int kk = 0; kk < kCcsgMaxClassTile; ++kk)
          if (kk < kt) {  // multiplied, never skipped: a NaN frame of zero saliency stays a NaN
            const double sv = sal ? ss[kk * FT + n] : 1.0;
            ar[kk] += sv * pr;
            ai[kk] += sv * pi;
          }
      }
#pragma unroll
      for (int kk = 0; kk < kCcsgMaxClassTile; ++kk)
        if (kk < kt) {
          if (G == 1)
            out[kk * Q + q] = make_double2(ar[kk], ai[kk]);
          else
            red[(g * kt + kk) * Q + q] = make_double2(ar[kk], ai[kk]);
        }
    }
    if (G > 1) {  // the slices, in ascending order
      __syncthreads();
      for (int p = tid; p < kt * Q; p += kFitThreads) {
        const int kk = p / Q, q = p - kk * Q;
        double2 acc = red[kk * Q + q];
        for (int g = 1; g < G; ++g) {
          acc.x += red[(g * kt + kk) * Q + q].x;
          acc.y += red[(g * kt + kk) * Q + q].y;
        }
        out[p] = acc;
      }
    }
  }
}

__global__ __launch_bounds__(256) void ccsg_fit_finish_kernel(const double2* part, int64_t total,
                                                              int64_t N, int D, int K, int spans,
                                                              int has_saliency, double floor,
                                                              double2* cov) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int tri = D * (D + 1) / 2, Q = tri + 1;
  const int64_t bk = i / tri;
  const int q = (int)(i - bk * tri);
  const int64_t b = bk / K;
  const int k = (int)(bk - b * K);
  const double2* p = part + (b * spans * K + k) * Q;
  double sr = 0.0, si = 0.0, den = 0.0;
  for (int sp = 0; sp < spans; ++sp, p += (int64_t)K * Q) {
    sr += p[q].x;
    si += p[q].y;
    den += p[tri].x;
  }
  if (has_saliency) den = den > floor ? den : floor;  // np.maximum(sum, tiny); a NaN sum stays
  else den = (double)N;
  int d = 0;
  while ((d + 1) * (d + 2) / 2 <= q) ++d;
  const int e = q - d * (d + 1) / 2;
  const double vr = sr / den, vi = d == e ? 0.0 : si / den;
  cov[(bk * D + d) * D + e] = make_double2(vr, vi);
  if (d != e) cov[(bk * D + e) * D + d] = make_double2(vr, -vi);
}

// -------------------------------------------------------------------------------------- log-pdf
// LDS: frames [NT * DS] complex128 | factors [KT * D * D] complex128 | reciprocal diagonals
// [KT * D] | offsets [KT] | flags [KT] (ccsg_frame_lds + KT * ccsg_class_lds bytes).
template <int DP, int NT>
__global__ __launch_bounds__(NT) void ccsg_log_pdf_kernel(const void* y, int c128, int64_t N,
                                                          int D, int K, int KT, int tiles,
                                                          const double2* cov, double* out_lp,
                                                          double* out_ld, int32_t* out_st) {
  extern __shared__ double2 ccsg_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int DS = D | 1, DD = D * D;
  const int64_t b = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - b * tiles);
  const int64_t n0 = (int64_t)tile * NT;
  const int nf = (int)(N - n0 < NT ? N - n0 : NT);
  double2* ys = ccsg_lds;
  double2* Lf = ys + NT * DS;
  double* invd = reinterpret_cast<double*>(Lf + KT * DD);
  double* off = invd + KT * D;
  int* flag = reinterpret_cast<int*>(off + KT);
  stage_frames<NT>(y, c128, (b * N + n0) * D, nf * D, D, DS, ys, tid);
  for (int k0 = 0; k0 < K; k0 += KT) {
    const int kt = K - k0 < KT ? K - k0 : KT;
    __syncthreads();  // the sweeps of the previous class tile are done
    for (int c = tid; c < kt; c += NT) flag[c] = 0;
    __syncthreads();
    // the lower triangle and the real part of the diagonal; nothing else of the matrix is read
    const double2* src = cov + (b * K + k0) * DD;
    for (int e = tid; e < kt * DD; e += NT) {
      const int c = e / DD, rc = e - c * DD, r = rc / D, col = rc - r * D;
      double2 v = make_double2(0.0, 0.0);
      if (col <= r) {
        v = src[e];
        if (col == r) v.y = 0.0;
        if (!(isfinite(v.x) && isfinite(v.y))) flag[c] = (int)PBBSS_ST_NONFINITE;
      }
      Lf[e] = v;
    }
    __syncthreads();
    for (int c = wave; c < kt; c += NT / 64) {  // one wavefront per matrix, lane = row
      double2* L = Lf + c * DD;
      int st = flag[c];
      double logdet = 0.0;
      for (int j = 0; j < D && !st; ++j) {
        double sr = 0.0, si = 0.0;
        if (lane >= j && lane < D) {
          const double2 a = L[lane * D + j];
          sr = a.x;
          si = a.y;
          for (int i = 0; i < j; ++i) {  // - l_ri conj(l_ji)
            const double2 lr = L[lane * D + i], lj = L[j * D + i];
            sr -= lr.x * lj.x + lr.y * lj.y;
            si -= lr.y * lj.x - lr.x * lj.y;
          }
        }
        const double piv = __shfl(sr, j);
        if (!isfinite(piv)) {
          st = (int)PBBSS_ST_NONFINITE;
        } else if (!(piv > 0.0)) {
          st = (int)PBBSS_ST_NOT_POSDEF;
        } else {
          const double dj = sqrt(piv);
          if (lane == j) {
            L[j * D + j] = make_double2(dj, 0.0);
            invd[c * D + j] = 1.0 / dj;
          } else if (lane > j && lane < D) {
            L[lane * D + j] = make_double2(sr / dj, si / dj);
          }
          logdet += log(piv);
        }
        wave_lds_fence();
      }
      if (lane == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        off[c] = st ? nan : -(double)D * 1.1447298858494001741434 - logdet;  // D ln pi
        if (tile == 0) {
          out_st[b * K + k0 + c] = st;
          if (out_ld) out_ld[b * K + k0 + c] = st ? nan : logdet;
        }
      }
    }
    __syncthreads();
    if (tid < nf) {
      const double2* yrow = ys + tid * DS;
      for (int c = 0; c < kt; ++c) {
        const double2* L = Lf + c * DD;
        const double* id = invd + c * D;
        double zr[DP], zi[DP], quad = 0.0;
#pragma unroll
        for (int j = 0; j < DP; ++j) {
          if (j < D) {
            const double2 yv = yrow[j];
            double sr = yv.x, si = yv.y;
#pragma unroll
            for (int i = 0; i < j; ++i) {
              const double2 l = L[j * D + i];
              sr -= l.x * zr[i] - l.y * zi[i];
              si -= l.x * zi[i] + l.y * zr[i];
            }
            zr[j] = sr * id[j];
            zi[j] = si * id[j];
            quad += zr[j] * zr[j] + zi[j] * zi[j];
          }
        }
        out_lp[(b * K + k0 + c) * N + n0 + tid] = off[c] - quad;
      }
    }
  }
}

inline int hip_ok() { return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP; }

template <int DP, int NT>
int launch_log_pdf(const void* y, int c128, int64_t B, int64_t N, int D, int K, const double* cov,
                   double* out_lp, double* out_ld, int32_t* out_st, hipStream_t s) {
  const int KT = K < ccsg_class_tile(D) ? K : ccsg_class_tile(D);
  const size_t lds = ccsg_frame_lds(D) + (size_t)KT * ccsg_class_lds(D);
  const int64_t tiles = (N + NT - 1) / NT;
  auto* kfn = ccsg_log_pdf_kernel<DP, NT>;
  if (!raise_lds_attribute(kfn, lds)) return PBBSS_ERR_LDS_CAPACITY;
  hipLaunchKernelGGL(kfn, dim3((unsigned)(B * tiles)), dim3(NT), lds, s, y, c128, N, D, K, KT,
                     (int)tiles, reinterpret_cast<const double2*>(cov), out_lp, out_ld, out_st);
  return hip_ok();
}

// frames | saliencies of a class tile | slice sums of a class tile
size_t fit_lds(int D, int K) {
  const size_t ka = K < kCcsgMaxClassTile ? K : kCcsgMaxClassTile;
  const size_t Q = (size_t)D * (D + 1) / 2 + 1;
  const size_t G = Q < kFitThreads ? kFitThreads / Q : 1;
  const size_t sliced = G > 1 ? G * Q : 0;
  return ccsg_frame_lds(D) + ka * ccsg_frames(D) * 8 + ka * sliced * 16;
}

}  // namespace

size_t ccsg_fit_partials(int64_t B, int64_t N, int D, int K) {
  const int64_t spans = (N + ccsg_frames(D) - 1) / ccsg_frames(D);
  return (size_t)B * spans * K * (D * (D + 1) / 2 + 1);
}

int launch_ccsg_fit(const void* y, int y_is_c128, int64_t B, int64_t N, int D, int K,
                    const void* saliency, int saliency_is_f64, double floor, double* part,
                    double* out_cov, hipStream_t s) {
  const int64_t spans = (N + ccsg_frames(D) - 1) / ccsg_frames(D);
  const size_t lds = fit_lds(D, K);
  double2* p2 = reinterpret_cast<double2*>(part);
  const dim3 grid((unsigned)(B * spans)), block(kFitThreads);
  if (saliency && !saliency_is_f64) {
    auto* kfn = ccsg_fit_kernel<float>;
    if (!raise_lds_attribute(kfn, lds)) return PBBSS_ERR_LDS_CAPACITY;
    hipLaunchKernelGGL(kfn, grid, block, lds, s, y, y_is_c128, N, D, K, (int)spans,
                       static_cast<const float*>(saliency), p2);
  } else {
    auto* kfn = ccsg_fit_kernel<double>;
    if (!raise_lds_attribute(kfn, lds)) return PBBSS_ERR_LDS_CAPACITY;
    hipLaunchKernelGGL(kfn, grid, block, lds, s, y, y_is_c128, N, D, K, (int)spans,
                       static_cast<const double*>(saliency), p2);
  }
  const int64_t total = B * K * (D * (D + 1) / 2);
  hipLaunchKernelGGL(ccsg_fit_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     s, p2, total, N, D, K, (int)spans, saliency != nullptr, floor,
                     reinterpret_cast<double2*>(out_cov));
  return hip_ok();
}

int launch_ccsg_log_pdf(const void* y, int y_is_c128, int64_t B, int64_t N, int D, int K,
                        const double* cov, double* out_lp, double* out_log_det,
                        int32_t* out_status, hipStream_t s) {
  // the smallest unrolled sweep that holds D (kCcsgSweepD); its frame tile is that of every D it serves
  constexpr int D0 = kCcsgSweepD[0], D1 = kCcsgSweepD[1], D2 = kCcsgSweepD[2], D3 = kCcsgSweepD[3];
  static_assert(D3 == kCcsgMaxD && ccsg_frames(D0) == ccsg_frames(1) &&
                ccsg_frames(D1) == ccsg_frames(D0 + 1) && ccsg_frames(D2) == ccsg_frames(D1 + 1) &&
                ccsg_frames(D3) == ccsg_frames(D2 + 1));
  if (D <= D0)
    return launch_log_pdf<D0, ccsg_frames(D0)>(y, y_is_c128, B, N, D, K, cov, out_lp, out_log_det,
                                               out_status, s);
  if (D <= D1)
    return launch_log_pdf<D1, ccsg_frames(D1)>(y, y_is_c128, B, N, D, K, cov, out_lp, out_log_det,
                                               out_status, s);
  if (D <= D2)
    return launch_log_pdf<D2, ccsg_frames(D2)>(y, y_is_c128, B, N, D, K, cov, out_lp, out_log_det,
                                               out_status, s);
  return launch_log_pdf<D3, ccsg_frames(D3)>(y, y_is_c128, B, N, D, K, cov, out_lp, out_log_det,
                                             out_status, s);
}

}  // namespace pbbss
