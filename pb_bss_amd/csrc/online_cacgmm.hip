// Frame-recursive cACGMM mask estimator (include/pbbss.h, XV; pb_bss_amd.distribution
// recursive_cacgmm, OnlineCACGMM): the cACG M-step as a running mean with exponential forgetting,
// the inverse of every class covariance kept by a rank-one (Sherman-Morrison) update, its
// log-determinant by the matrix determinant lemma, a-priori masks per frame.
//
// One wavefront per problem, persistent over the frames of the call, and no workgroup barrier:
// the four wavefronts of a workgroup never meet.  The K precisions live in registers on the lane
// grid of lane_grid.hpp, Hermitian to the bit.
//
// The scalars of a class (weight, its logarithm, log-determinant, count) live on the lanes l with
// l % 8 == k: the logarithms, the exponential and the divisions of a frame are computed once for
// all classes, not once per class; the softmax and the sum of the counts are 8-lane DPP trees, the
// two factors of the update go back to all lanes through v_readlane.
//
// Frames are staged a tile ahead (frame_tile.hpp); at the tile's start lanes 0..31 take the norm
// of a frame each (sensors in ascending order) and the tile is divided by it.  Per frame, with
// z = y / nu:
//   n_k = P_k z: E products per lane and class, row sums by DPP -- a fixed tree;
//   q_k = Re(z^H n_k): K interleaved 64-lane DPP / permlane-swap trees;
//   lp = log pi - L - D log q, gamma = softmax(lp), clipped; old = alpha Lambda,
//   new = old + gamma, den = old + D gamma on the class lanes;
//   P_k <- (P_k - ((D gamma / (q den)) n) n^H) (new / old);
//   L += D log(old / new) + log(den / old); Lambda = new; pi = Lambda / sum Lambda.
// q or old not > 0, or a non-finite q, gamma, L or Lambda, stops the recursion of that problem:
// gamma and q from that frame on, P, L, Lambda and pi are NaN and the status word is set.
#include "online_cacgmm.hpp"
#include <float.h>
#include <math.h>
#include "dispatch.hpp"
#include "frame_tile.hpp"
#include "lane_grid.hpp"

namespace pbbss {
namespace {

constexpr int kTile = kOnlineCacgmmTile;
constexpr int kWaves = kOnlineCacgmmWaves;
constexpr int kGroup = kOnlineCacgmmMaxK;  // lanes of a class group
static_assert(kTile == 32 && kGroup == 8, "lanes 0..31 take a norm each; 8-lane DPP trees");

template <int E>
struct FrameIn {
  double2 zr, zc[E];
  double nu;
};

template <int DB, int K>
__global__ __launch_bounds__(kWaves * kWave) void online_cacgmm_kernel(WpeFrames y,
                                                                       OnlineCacgmmArgs a,
                                                                       int64_t B) {
  using Grid = LaneGrid<DB>;
  constexpr int LPR = Grid::LPR, E = Grid::E;
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
  const int D = y.D;
  const Grid g(lane, D);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double alpha = a.alpha, eps = a.affiliation_eps, Dd = (double)D;
  const bool clip = eps > 0.0, uw = a.update_weight != 0;

  // ---- the precisions
  double2 psi[K][E];
  auto P = [&](int k) { return reinterpret_cast<double2*>(a.precision) + (b * K + k) * D * D; };
#pragma unroll
  for (int k = 0; k < K; ++k) g.load_hermitian(P(k), D, psi[k]);
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

  TilePrefetch<kTile, DB, kWave> pre;
  auto read = [&](int u) {
    FrameIn<E> f;
    g.read_frame(fr, u, f.zr, f.zc);
    f.nu = nus[u];
    return f;
  };
  pre.fetch(y, b, 0, lane);

  for (int64_t t0 = 0; t0 < T; t0 += kTile) {
    const int nf = pre.frames(T, t0);
    pre.stage(y, t0, lane, fr, [](int u, int d) { return u * DB + d; });
    wave_lds_order();
    if (t0 + kTile < T) pre.fetch(y, b, t0 + kTile, lane);  // in flight during this tile's frames
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
    for (int i = 0; i < pre.kPre; ++i) {
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
      const double top = lanes8_max(lp);
      const double ex0 = exp_nonpos(lp - top);
      const double ex = valid ? ex0 : 0.0;
      const double graw = ex / lanes8_sum(ex);
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
      // ---- P_k <- (P_k - (coef_k n_k) n_k^H) scale_k
#pragma unroll
      for (int k = 0; k < K; ++k)
        g.downdate(psi[k], nr[k], ni[k], lane_const(coef, k), lane_const(scale, k));
      L_c = Ln;
      Lam_c = nw;
      if (uw) {
        pi_c = Lam_c / lanes8_sum(valid ? Lam_c : 0.0);
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

#pragma unroll
  for (int k = 0; k < K; ++k) g.store_hermitian(P(k), D, psi[k], dead);
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
