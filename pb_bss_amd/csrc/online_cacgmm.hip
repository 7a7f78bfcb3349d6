// Frame-recursive cACGMM mask estimator (include/pbbss.h, XV; pb_bss_amd.distribution
// recursive_cacgmm, OnlineCACGMM): the cACG M-step as a running mean with exponential forgetting,
// the inverse of every class covariance kept by a rank-one (Sherman-Morrison) update, its
// log-determinant by the matrix determinant lemma, a-priori masks per frame.
//
// One wavefront per problem, persistent over the frames of the call, and no workgroup barrier:
// the four wavefronts of a workgroup never meet.  The lane grid is that of online_bf.hip -- lane l
// owns row l / LPR and the columns l % LPR + e LPR, e < E, with (LPR, E) = (4, 1), (8, 1), (4, 4)
// for the sensor bounds 4, 8, 16 -- and carries the K precisions as FULL matrices in registers:
// every lane computes the element of the LOWER triangle that it owns or mirrors with the same
// instructions on the same values as its mirror lane and stores the conjugate above the diagonal,
// so the upper triangle is the conjugate mirror to the bit.  Rows and columns beyond D hold zeros.
//
// The scalars of a class (weight, its logarithm, log-determinant, count) live on the lanes l with
// l % 8 == k: the logarithms, the exponential and the divisions of a frame are computed once for
// all classes, not once per class; the softmax and the sum of the counts are 8-lane DPP trees, the
// two factors of the update go back to all lanes through v_readlane.
//
// Frames are staged a tile ahead in registers and handed to the wavefront's own slice of LDS at
// the tile's start, where lanes 0..31 take the norm of a frame each (sensors in ascending order)
// and the tile is divided by it.  Per frame, with z = y / nu:
//   n_k = P_k z: E products per lane and class, row sums by DPP -- a fixed tree;
//   q_k = Re(z^H n_k): K interleaved 64-lane DPP / permlane-swap trees;
//   lp = log pi - L - D log q, gamma = softmax(lp), clipped; old = alpha Lambda,
//   new = old + gamma, den = old + D gamma on the class lanes;
//   n_c from the lanes of row c; P_k <- (P_k - ((D gamma / (q den)) n) n^H) (new / old);
//   L += D log(old / new) + log(den / old); Lambda = new; pi = Lambda / sum Lambda.
// q or old not > 0, or a non-finite q, gamma, L or Lambda, stops the recursion of that problem:
// gamma and q from that frame on, P, L, Lambda and pi are NaN and the status word is set.
#include "online_cacgmm.hpp"
#include <float.h>
#include <math.h>
#include "dispatch.hpp"
#include "pbbss_dev.hpp"

namespace pbbss {
namespace {

constexpr int kTile = kOnlineCacgmmTile;
constexpr int kWaves = kOnlineCacgmmWaves;
constexpr int kGroup = kOnlineCacgmmMaxK;  // lanes of a class group
static_assert(kTile == 32 && kGroup == 8, "lanes 0..31 take a norm each; 8-lane DPP trees");

__device__ __forceinline__ double2 load_frame(const WpeFrames& y, int64_t i) {
  if (y.c128) return static_cast<const double2*>(y.p)[i];
  const float2 v = static_cast<const float2*>(y.p)[i];
  return make_double2((double)v.x, (double)v.y);
}

// element idx of a tile of nf frames -> (sensor, frame); the inner index is the axis that is
// contiguous in memory
struct TileAt {
  int d, u;
};
__device__ __forceinline__ TileAt tile_index(const WpeFrames& y, int idx, int nf) {
  const bool sensors_inner = y.sd == 1 && y.D > 1;
  const int q = idx / (sensors_inner ? y.D : nf), m = idx - q * (sensors_inner ? y.D : nf);
  return sensors_inner ? TileAt{m, q} : TileAt{q, m};
}

// The lanes of a wavefront read LDS that other lanes of the same wavefront wrote: the hardware
// keeps a wavefront's LDS operations in order, this keeps the compiler from reordering them.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum over the LPR lanes of a row of the lane grid, on every lane of the row, for K classes
template <int LPR, int K>
__device__ __forceinline__ void row_sums(double (&a)[K], double (&b)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    a[k] += dpp_mov_f64<kDppQuadXor1>(a[k]);
    b[k] += dpp_mov_f64<kDppQuadXor1>(b[k]);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    a[k] += dpp_mov_f64<kDppQuadXor2>(a[k]);
    b[k] += dpp_mov_f64<kDppQuadXor2>(b[k]);
  }
  if constexpr (LPR == 8) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      a[k] += dpp_mov_f64<kDppRowHalfMirror>(a[k]);
      b[k] += dpp_mov_f64<kDppRowHalfMirror>(b[k]);
    }
  }
}

// K sums over the 64 lanes, on every lane: the tree of wave_sum, stage by stage for all classes
template <int K>
__device__ __forceinline__ void wave_sums(double (&v)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] += dpp_mov_f64<kDppQuadXor1>(v[k]);
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] += dpp_mov_f64<kDppQuadXor2>(v[k]);
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] += dpp_mov_f64<kDppRowHalfMirror>(v[k]);
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] += dpp_mov_f64<kDppRowMirror>(v[k]);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double a = v[k], b = v[k];
    swap16_f64(a, b);
    v[k] = a + b;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double a = v[k], b = v[k];
    swap32_f64(a, b);
    v[k] = a + b;
  }
}

// over the 8 lanes of a class group, on every lane of the group
__device__ __forceinline__ double group_sum(double v) {
  v += dpp_mov_f64<kDppQuadXor1>(v);
  v += dpp_mov_f64<kDppQuadXor2>(v);
  return v + dpp_mov_f64<kDppRowHalfMirror>(v);
}
__device__ __forceinline__ double group_max(double v) {
  v = fmax(v, dpp_mov_f64<kDppQuadXor1>(v));
  v = fmax(v, dpp_mov_f64<kDppQuadXor2>(v));
  return fmax(v, dpp_mov_f64<kDppRowHalfMirror>(v));
}

// the value of lane `src` (a constant below 8) on every lane, through scalar registers
__device__ __forceinline__ double lane_const(double v, int src) {
  F64Bits s, r;
  s.d = v;
  r.i[0] = __builtin_amdgcn_readlane(s.i[0], src);
  r.i[1] = __builtin_amdgcn_readlane(s.i[1], src);
  return r.d;
}

template <int E>
struct FrameIn {
  double2 zr, zc[E];
  double nu;
};

template <int DB, int K>
__global__ __launch_bounds__(kWaves * kWave) void online_cacgmm_kernel(WpeFrames y,
                                                                       OnlineCacgmmArgs a,
                                                                       int64_t B) {
  constexpr int LPR = DB == 8 ? 8 : 4;      // lanes per row of the lane grid
  constexpr int E = DB / LPR;               // columns per lane
  constexpr int kPre = kTile * DB / kWave;  // elements of a tile per lane
  static_assert(LPR * DB <= kWave && E * LPR == DB && kPre * kWave == kTile * DB);
  static_assert(K >= 2 && K <= kGroup);
  __shared__ double2 fr_s[kWaves][kTile * DB];  // [frame][sensor], zeros beyond D
  __shared__ double nu_s[kWaves][kTile];
  __shared__ double go_s[kWaves][2 * K * kTile];  // gamma [class][frame] | q [class][frame]
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t b = (int64_t)blockIdx.x * kWaves + wave, T = y.T;
  if (b >= B) return;  // whole wavefronts: nobody waits for them
  double2* fr = fr_s[wave];
  double* nus = nu_s[wave];
  double* go = go_s[wave];
  double* qo = go + K * kTile;
  const int D = y.D, r = lane / LPR, cl = lane - r * LPR;
  const bool rowok = r < D;
  const int rr = rowok ? r : 0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double alpha = a.alpha, eps = a.affiliation_eps, Dd = (double)D;
  const bool clip = eps > 0.0, uw = a.update_weight != 0;

  // ---- the precisions: the lower triangle and the real diagonal are read
  double2 psi[K][E];
  bool lower[E], diag[E], act[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int c = cl + e * LPR;
    act[e] = rowok && c < D;
    lower[e] = r >= c;
    diag[e] = r == c;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double2* P = reinterpret_cast<const double2*>(a.precision) + (b * K + k) * D * D;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int c = cl + e * LPR;
      psi[k][e] = make_double2(0.0, 0.0);
      if (act[e]) {
        psi[k][e] = P[lower[e] ? r * D + c : c * D + r];
        if (!lower[e]) psi[k][e].y = -psi[k][e].y;
        if (diag[e]) psi[k][e].y = 0.0;
      }
    }
  }
  // ---- the scalars of class lane % 8, on every lane of that residue
  const int kc = lane & (kGroup - 1);
  const bool valid = kc < K, writer = lane < K;
  double pi_c = 1.0, L_c = 0.0, Lam_c = 1.0;
  if (valid) {
    pi_c = a.weight[b * K + kc];
    L_c = a.log_determinant[b * K + kc];
    Lam_c = a.count[b * K + kc];
  }
  double logpi_c = log_pos(pi_c);
  for (int i = lane; i < kTile * DB; i += kWave) fr[i] = make_double2(0.0, 0.0);
  const int64_t seen = a.frames_seen[b];
  bool dead = false;

  double2 pre[kPre];
  auto fetch = [&](int64_t t0) {
    const int nf = (int)(T - t0 < kTile ? T - t0 : kTile);
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
      const int idx = lane + kWave * i;
      pre[i] = make_double2(0.0, 0.0);
      if (idx < nf * D) {
        const TileAt at = tile_index(y, idx, nf);
        pre[i] = load_frame(y, b * y.sb + at.d * y.sd + (t0 + at.u) * y.st);
      }
    }
  };
  auto read = [&](int u) {
    FrameIn<E> f;
    const double2 v = fr[u * DB + rr];
    f.zr = rowok ? v : make_double2(0.0, 0.0);
#pragma unroll
    for (int e = 0; e < E; ++e) f.zc[e] = fr[u * DB + cl + e * LPR];
    f.nu = nus[u];
    return f;
  };
  fetch(0);

  for (int64_t t0 = 0; t0 < T; t0 += kTile) {
    const int nf = (int)(T - t0 < kTile ? T - t0 : kTile);
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
      const int idx = lane + kWave * i;
      if (idx < nf * D) {
        const TileAt at = tile_index(y, idx, nf);
        fr[at.u * DB + at.d] = pre[i];
      }
    }
    wave_lds_order();
    if (t0 + kTile < T) fetch(t0 + kTile);  // in flight during the frames of this tile
    // ---- nu of a frame per lane, the sensors in ascending order; then z = y / nu in place
    if (lane < nf) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        const double2 v = fr[lane * DB + d];
        s += v.x * v.x + v.y * v.y;
      }
      nus[lane] = sqrt(s);
    }
    wave_lds_order();
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
      const int p = lane + kWave * i, u = p / DB, d = p - u * DB;
      if (u < nf && d < D) {
        const double nu = nus[u];
        if (nu != 0.0) {
          const double2 v = fr[p];
          fr[p] = make_double2(v.x / nu, v.y / nu);
        }
      }
    }
    wave_lds_order();

    FrameIn<E> nxt = read(0);
    for (int u = 0; u < nf; ++u) {
      const FrameIn<E> f = nxt;
      nxt = read(u + 1 < kTile ? u + 1 : u);  // a frame ahead of its use
      if (dead) {
        if (writer) go[kc * kTile + u] = nan, qo[kc * kTile + u] = nan;
        continue;
      }
      if (f.nu == 0.0) {  // an all-zero frame: the prior, and the state is not touched
        if (writer) go[kc * kTile + u] = pi_c, qo[kc * kTile + u] = 0.0;
        continue;
      }
      // ---- n_k = P_k z and q_k = Re(z^H n_k)
      double nr[K], ni[K], q[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        nr[k] = ni[k] = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          nr[k] += psi[k][e].x * f.zc[e].x - psi[k][e].y * f.zc[e].y;
          ni[k] += psi[k][e].x * f.zc[e].y + psi[k][e].y * f.zc[e].x;
        }
        q[k] = f.zr.x * nr[k] + f.zr.y * ni[k];
      }
      wave_sums<K>(q);
      row_sums<LPR, K>(nr, ni);
      // ---- the class lanes: posterior, counts, the two factors of the update
      double myq = q[0];
#pragma unroll
      for (int k = 1; k < K; ++k) myq = kc == k ? q[k] : myq;
      const double old = alpha * Lam_c;
      const double lp = valid ? logpi_c - L_c - Dd * log_pos(myq) : -INFINITY;
      // (the cross-lane trees stay outside every lane-dependent condition: DPP reads no idle lane)
      const double top = group_max(lp);
      const double ex0 = exp_nonpos(lp - top);
      const double ex = valid ? ex0 : 0.0;
      const double graw = ex / group_sum(ex);
      const double gam = clip ? fmin(fmax(graw, eps), 1.0 - eps) : graw;
      const double nw = old + gam, den = old + Dd * gam;
      const double Ln = L_c + Dd * log_pos(old / nw) + log_pos(den / old);
      const bool bad = valid && !(myq > 0.0 && old > 0.0 && isfinite(myq) && isfinite(graw) &&
                                  isfinite(Ln) && isfinite(nw));
      if (__builtin_amdgcn_ballot_w64(bad) != 0) {  // the same in every lane
        dead = true;                                // from this frame on
        if (writer) go[kc * kTile + u] = nan, qo[kc * kTile + u] = nan;
        continue;
      }
      if (writer) go[kc * kTile + u] = gam, qo[kc * kTile + u] = myq;
      const double coef = Dd * gam / (myq * den), scale = nw / old;
      // ---- P_k <- (P_k - (coef n) n^H) scale, the element (max(r, c), min(r, c)) on either lane
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double ck = lane_const(coef, k), sk = lane_const(scale, k);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int src = (cl + e * LPR) * LPR;  // a lane of row c
          const double cr = lane_get(nr[k], src), ci = lane_get(ni[k], src);
          const double Rr = lower[e] ? nr[k] : cr, Ri = lower[e] ? ni[k] : ci;
          const double Cr = lower[e] ? cr : nr[k], Ci = lower[e] ? ci : ni[k];
          const double kx = Rr * ck, ky = Ri * ck;
          double ly = lower[e] ? psi[k][e].y : -psi[k][e].y;
          psi[k][e].x = (psi[k][e].x - (kx * Cr + ky * Ci)) * sk;
          ly = diag[e] ? 0.0 : (ly - (ky * Cr - kx * Ci)) * sk;
          psi[k][e].y = lower[e] ? ly : -ly;
        }
      }
      L_c = Ln;
      Lam_c = nw;
      if (uw) {
        pi_c = Lam_c / group_sum(valid ? Lam_c : 0.0);
        logpi_c = log_pos(pi_c);
      }
    }
    // ---- the tile of gamma and q
    wave_lds_order();
    for (int i = lane; i < K * kTile; i += kWave) {
      const int k = i / kTile, u = i - k * kTile;
      if (u < nf) {
        const int64_t at = (b * K + k) * T + t0 + u;
        a.out_affiliation[at] = go[i];
        if (a.out_q) a.out_q[at] = qo[i];
      }
    }
    wave_lds_order();
  }

  // ---- the state: the whole matrices, Hermitian to the bit
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double2* P = reinterpret_cast<double2*>(a.precision) + (b * K + k) * D * D;
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (act[e]) P[r * D + cl + e * LPR] = dead ? make_double2(nan, nan) : psi[k][e];
  }
  if (writer) {
    a.weight[b * K + kc] = dead ? nan : pi_c;
    a.log_determinant[b * K + kc] = dead ? nan : L_c;
    a.count[b * K + kc] = dead ? nan : Lam_c;
  }
  if (lane == 0) {
    a.frames_seen[b] = seen + T;
    a.status[b] = dead ? (int32_t)PBBSS_ST_NONFINITE : 0;
  }
}

}  // namespace

int launch_online_cacgmm(const WpeFrames& y, int64_t B, const OnlineCacgmmArgs& a, hipStream_t s) {
  constexpr int D0 = kOnlineCacgmmD[0], D1 = kOnlineCacgmmD[1], D2 = kOnlineCacgmmD[2];
  static_assert(D2 == kOnlineCacgmmMaxD);
  return dispatch_list<D0, D1, D2>(y.D <= D0 ? D0 : y.D <= D1 ? D1 : D2, [&](auto dp) {
    return dispatch_range<2, kOnlineCacgmmMaxK>(a.K, [&](auto kp) {
      hipLaunchKernelGGL((online_cacgmm_kernel<decltype(dp)::value, decltype(kp)::value>),
                         dim3((unsigned)((B + kWaves - 1) / kWaves)), dim3(kWaves * kWave), 0, s,
                         y, a, B);
      return hipGetLastError() == hipSuccess ? (int)PBBSS_OK : (int)PBBSS_ERR_HIP;
    });
  });
}

}  // namespace pbbss
