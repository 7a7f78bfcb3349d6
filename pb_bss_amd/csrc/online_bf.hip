// Frame-recursive mask-driven MVDR (include/pbbss.h, XIV; pb_bss_amd.extraction
// recursive_mvdr_souden, OnlineMVDR): exponentially forgotten target statistics, the noise inverse
// kept by a rank-one (Sherman-Morrison) update, the Souden vector and its output per frame.
//
// One wavefront per problem, persistent over the frames of the call, and no workgroup barrier:
// the four wavefronts of a workgroup never meet.  Phi and Psi live in registers on the lane grid
// of lane_grid.hpp, Hermitian to the bit.
//
// Frames and masks are staged a tile ahead (frame_tile.hpp); a frame's y_r, y_c and masks are read
// from LDS one frame ahead of their use.  Per frame:
//   Phi <- alpha Phi + s y y^H
//   n = Psi y: E products per lane, row sums by DPP;
//   den = alpha + v Re(y^H n): the 64-lane DPP / permlane-swap tree over Re(conj(y_r) p_lane);
//   Psi <- (Psi - (v / den) n n^H) / alpha
//   u = Phi[:, ref] as conj(Phi[ref, c]) from the lanes of row ref; q = Psi u by row sums;
//   lam = sum Re(Psi_ij conj(Phi_ij)) on the 64-lane tree; w = q / max(lam, tiny); x = w^H y on
//   the 64-lane tree.
// den not > 0, or a non-finite den, lam or x, stops the recursion of that problem: x and w from
// that frame on, Phi and Psi are NaN and the status word is set.  (A non-finite element of Phi or
// Psi makes lam non-finite in the same frame: 0 * inf is NaN.)
#include "online_bf.hpp"
#include <float.h>
#include <math.h>
#include "dispatch.hpp"
#include "frame_tile.hpp"
#include "lane_grid.hpp"

namespace pbbss {
namespace {

constexpr int kTile = kOnlineBfTile;
constexpr int kWaves = kOnlineBfWaves;
static_assert(kTile == 32, "one lane per frame and mask: lanes 0..31 target, 32..63 noise");

template <int E>
struct FrameIn {
  double2 yr, yc[E];
  double s, v;
};

template <int DB>
__global__ __launch_bounds__(kWaves * kWave) void online_mvdr_kernel(WpeFrames y, OnlineBfArgs a,
                                                                     int64_t B) {
  using Grid = LaneGrid<DB>;
  constexpr int LPR = Grid::LPR, E = Grid::E;
  __shared__ double2 fr_s[kWaves][kTile * DB];  // [frame][sensor], zeros beyond D
  __shared__ double2 xo_s[kWaves][kTile];
  __shared__ double mk_s[kWaves][2 * kTile];    // target masks | noise masks
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t b = (int64_t)blockIdx.x * kWaves + wave, T = y.T;
  if (b >= B) return;  // whole wavefronts: nobody waits for them
  double2* fr = fr_s[wave];
  double2* xo = xo_s[wave];
  double* mk = mk_s[wave];
  const int D = y.D;
  const Grid g(lane, D);
  const bool head = g.rowok && g.cl == 0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double alpha = a.alpha, inv_alpha = 1.0 / a.alpha;

  // ---- the state
  double2 phi[E], psi[E];
  double2* Phi = reinterpret_cast<double2*>(a.target_psd) + b * D * D;
  double2* Psi = reinterpret_cast<double2*>(a.noise_inv) + b * D * D;
  g.load_hermitian(Phi, D, phi);
  g.load_hermitian(Psi, D, psi);
  for (int i = lane; i < kTile * DB; i += kWave) fr[i] = make_double2(0.0, 0.0);
  const int64_t seen = a.frames_seen[b];
  bool dead = false;

  TilePrefetch<kTile, DB, kWave> pre;
  double mpre = 0.0;
  auto fetch = [&](int64_t t0) {
    pre.fetch(y, b, t0, lane);
    const int u = lane & (kTile - 1);
    mpre = 0.0;
    if (u < pre.frames(T, t0)) {
      const void* m = lane < kTile ? a.target_mask : a.noise_mask;
      const int64_t at = b * T + t0 + u;
      mpre = a.mask_f64 ? static_cast<const double*>(m)[at]
                        : (double)static_cast<const float*>(m)[at];
    }
  };
  auto read = [&](int u) {
    FrameIn<E> f;
    g.read_frame(fr, u, f.yr, f.yc);
    f.s = mk[u];
    f.v = mk[kTile + u];
    return f;
  };
  fetch(0);

  for (int64_t t0 = 0; t0 < T; t0 += kTile) {
    const int nf = pre.frames(T, t0);
    pre.stage(y, t0, lane, fr, [](int u, int d) { return u * DB + d; });
    mk[lane] = mpre;
    wave_lds_order();
    if (t0 + kTile < T) fetch(t0 + kTile);  // in flight during the frames of this tile

    FrameIn<E> nxt = read(0);
    for (int u = 0; u < nf; ++u) {
      const FrameIn<E> f = nxt;
      nxt = read(u + 1 < kTile ? u + 1 : u);  // a frame ahead of its use
      double2* wo = a.out_w ? reinterpret_cast<double2*>(a.out_w) + ((t0 + u) * B + b) * D + g.r
                            : nullptr;
      if (dead) {
        if (lane == 0) xo[u] = make_double2(nan, nan);
        if (wo && head) *wo = make_double2(nan, nan);
        continue;
      }
      // ---- Phi <- alpha Phi + s y y^H, the element (max(r, c), min(r, c)) on either lane
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const double2 p = g.lower[k] ? f.yr : f.yc[k], q = g.lower[k] ? f.yc[k] : f.yr;
        const double re = p.x * q.x + p.y * q.y, im = p.y * q.x - p.x * q.y;
        double ly = g.lower[k] ? phi[k].y : -phi[k].y;
        phi[k].x = alpha * phi[k].x + f.s * re;
        ly = g.diag[k] ? 0.0 : alpha * ly + f.s * im;
        phi[k].y = g.lower[k] ? ly : -ly;
      }
      // ---- n = Psi y and den = alpha + v Re(y^H n)
      double nr = 0.0, ni = 0.0;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        nr += psi[k].x * f.yc[k].x - psi[k].y * f.yc[k].y;
        ni += psi[k].x * f.yc[k].y + psi[k].y * f.yc[k].x;
      }
      const double den = alpha + f.v * wave_sum(f.yr.x * nr + f.yr.y * ni);
      row_sums<LPR, 1>(&nr, &ni);
      if (!(den > 0.0) || !isfinite(den)) {  // the same value in every lane
        dead = true;  // from this frame on
        if (lane == 0) xo[u] = make_double2(nan, nan);
        if (wo && head) *wo = make_double2(nan, nan);
        continue;
      }
      // ---- Psi <- (Psi - (v / den) n n^H) / alpha
      g.downdate(psi, nr, ni, f.v / den, inv_alpha);
      // ---- the Souden vector of the statistics that include this frame
      double qr = 0.0, qi = 0.0, lam = 0.0;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        const int src = a.ref * LPR + g.cl;  // Phi[ref, c]: its conjugate is u_c = Phi[c, ref]
        const double ur = lane_get(phi[k].x, src), ui = -lane_get(phi[k].y, src);
        qr += psi[k].x * ur - psi[k].y * ui;
        qi += psi[k].x * ui + psi[k].y * ur;
        lam += psi[k].x * phi[k].x + psi[k].y * phi[k].y;
      }
      row_sums<LPR, 1>(&qr, &qi);
      lam = wave_sum(lam);
      const double rl = 1.0 / fmax(lam, DBL_MIN);
      double2 w = make_double2(qr * rl, qi * rl);
      double xr = head ? w.x * f.yr.x + w.y * f.yr.y : 0.0;  // conj(w_r) y_r
      double xi = head ? w.x * f.yr.y - w.y * f.yr.x : 0.0;
      xr = wave_sum(xr);
      xi = wave_sum(xi);
      if (!(isfinite(lam) && isfinite(xr) && isfinite(xi))) {
        dead = true;
        xr = xi = nan;
        w = make_double2(nan, nan);
      }
      if (lane == 0) xo[u] = make_double2(xr, xi);
      if (wo && head) *wo = w;
    }
    // ---- the tile of x, with the type of y
    wave_lds_order();
    if (lane < nf) {
      const double2 x = xo[lane];
      const int64_t i = b * T + t0 + lane;
      if (y.c128)
        static_cast<double2*>(a.out_x)[i] = x;
      else
        static_cast<float2*>(a.out_x)[i] = make_float2((float)x.x, (float)x.y);
    }
    wave_lds_order();
  }

  g.store_hermitian(Phi, D, phi, dead);
  g.store_hermitian(Psi, D, psi, dead);
  if (lane == 0) {
    a.frames_seen[b] = seen + T;
    a.status[b] = dead ? (int32_t)PBBSS_ST_NONFINITE : 0;
  }
}

}  // namespace

int launch_online_mvdr(const WpeFrames& y, int64_t B, const OnlineBfArgs& a, hipStream_t s) {
  auto run = [&](auto dp) {
    hipLaunchKernelGGL(online_mvdr_kernel<decltype(dp)::value>,
                       dim3((unsigned)((B + kWaves - 1) / kWaves)), dim3(kWaves * kWave), 0, s, y,
                       a, B);
    return hipGetLastError() == hipSuccess ? (int)PBBSS_OK : (int)PBBSS_ERR_HIP;
  };
  constexpr int D0 = kOnlineBfD[0], D1 = kOnlineBfD[1], D2 = kOnlineBfD[2];
  static_assert(D2 == kOnlineBfMaxD);
  return dispatch_list<D0, D1, D2>(y.D <= D0 ? D0 : y.D <= D1 ? D1 : D2, run);
}

}  // namespace pbbss
