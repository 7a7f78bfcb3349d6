// Frame-recursive (online) WPE (include/pbbss.h, XIII; nara_wpe.wpe: online_wpe_step,
// recursive_wpe, OnlineWPE): one recursive-least-squares update of the prediction filter per
// frame.  One workgroup per problem, persistent over the frames of the call; the M x M inverse
// covariance P lives in LDS as a packed lower triangle (the upper one is its conjugate mirror by
// definition), beside the filter G and the last taps + delay frames.
//
// Frames are kept newest first, [slot][D]: tile frame u lies in slot kTile - 1 - u, the frame j
// before the tile in slot kTile - 1 + j.  The stacked past of frame u (tap k of sensor d at
// k D + d, frame u - delay - k) is then the M consecutive elements from slot
// kTile - 1 - u + delay on: nothing is gathered.  After a tile the newest taps + delay frames move
// up behind it; the next tile waits in registers meanwhile, so no global load is on the per-frame
// chain, and a frame is read from global memory once.
//
// Per frame, two workgroup barriers:
//   A  M + D dot products of length M with the stacked past: n = P ytilde (row r reads
//      L[r][c <= r] and conj(L[c > r][r])) and x = y - G^H ytilde.  S lanes share a row and add
//      their partial sums on a fixed xor tree.                                        -- barrier
//   B  den = alpha lambda + Re(ytilde^H n): every wavefront sums the M terms on the same xor tree
//      (no barrier for a broadcast); 1 / den, or 0 where den is not > 0.
//   C  P <- (P - k n^H) / alpha on the triangle, rows r and M - 1 - r paired so that every group
//      of lanes has M + 1 elements; G <- G + k x^H.                                   -- barrier
// A non-finite den or x stops the recursion of that problem: the output from that frame on is
// NaN, P and G are written back as NaN and the status word is set; a non-finite element written
// to P or G shows in den or x of the next frame, or in the flag every lane keeps for the end of
// the call.
#include "wpe_online.hpp"
#include <math.h>
#include "frame_tile.hpp"
#include "launch_util.hpp"

namespace pbbss {
namespace {

constexpr int kTile = kWpeOnlineTile;

// a __shfl_xor butterfly, not the DPP tree of pbbss_dev.hpp's wave_sum: it adds in another order
__device__ __forceinline__ double wave_sum_xor(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct OnlineArgs {
  int taps, delay;
  double alpha, inv_alpha;
  const double* power;
  double2 *P, *G, *hist;
  int64_t* seen;
  void* out_x;
  int32_t* status;
};

constexpr int NT = kWpeOnlineThreads;

__global__ __launch_bounds__(NT) void wpe_online_kernel(WpeFrames y, OnlineArgs a) {
  extern __shared__ double2 wpe_online_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int D = y.D, M = D * a.taps, Me = M + D, H = a.taps + a.delay;
  const int tri = M * (M + 1) / 2;
  const int64_t b = blockIdx.x, T = y.T;
  double2* L = wpe_online_lds;
  double2* Gs = L + tri;
  double2* fr = Gs + M * D;
  double2* xo = fr + (H + kTile) * D;
  double2* nv = xo + kTile * D;
  double2* xs = nv + M;
  double* lam = reinterpret_cast<double*>(xs + kWpeMaxD);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  // lanes per dot product of stage A: a power of two, so that a row never straddles a wavefront
  int S = 1;
  while (2 * S * Me <= NT && S < 64) S *= 2;
  const int a_row = tid / S, a_sub = tid - a_row * S, a_step = NT / S;
  // stage C: NP pairs of rows (r, M - 1 - r), S2 lanes per pair
  const int NP = (M + 1) / 2;
  const int S2 = NT / NP > 0 ? NT / NP : 1;
  const int c_pair = tid / S2, c_sub = tid - c_pair * S2, c_step = NT / S2;
  // the update of G: lane (m, d) on a grid whose width is the power of two that holds D
  int DP = 1, dshift = 0;
  while (DP < D) DP *= 2, ++dshift;
  const int g_d = tid & (DP - 1), g_m = tid >> dshift, g_step = NT >> dshift;

  // ---- the state
  const double2* Pb = a.P + b * M * M;
  for (int e = tid; e < M * M; e += NT) {
    const int r = e / M, c = e - r * M;
    if (c <= r) {
      double2 v = Pb[e];
      if (c == r) v.y = 0.0;
      L[r * (r + 1) / 2 + c] = v;
    }
  }
  for (int e = tid; e < M * D; e += NT) Gs[e] = a.G[b * M * D + e];
  for (int e = tid; e < H * D; e += NT) {  // history (D, H), newest last
    const int d = e / H, i = e - d * H;
    fr[(kTile + H - 1 - i) * D + d] = a.hist[(b * D + d) * H + i];
  }
  const int64_t seen = a.seen[b];
  bool dead = false;
  int bad = 0;

  TilePrefetch<kTile, kWpeMaxD, NT> pre;
  pre.fetch(y, b, 0, tid);

  for (int64_t t0 = 0; t0 < T; t0 += kTile) {
    const int nf = pre.frames(T, t0);
    pre.stage(y, t0, tid, fr, [D](int u, int d) { return (kTile - 1 - u) * D + d; });
    __syncthreads();
    if (t0 + kTile < T) pre.fetch(y, b, t0 + kTile, tid);  // in flight during this tile's frames
    if (tid < nf) {
      const int u = tid;
      if (a.power) {
        lam[u] = a.power[b * T + t0 + u];
      } else {  // the frames u - H .. u in ascending order; those before the stream are zeros
        double s = 0.0;
        for (int slot = kTile - 1 - u + H; slot >= kTile - 1 - u; --slot) {
          double pf = 0.0;
          for (int d = 0; d < D; ++d) {
            const double2 v = fr[slot * D + d];
            pf += v.x * v.x + v.y * v.y;
          }
          s += pf;
        }
        const int64_t have = seen + t0 + u + 1;
        lam[u] = s / (double)(D * (have < H + 1 ? have : H + 1));
      }
    }
    __syncthreads();

    for (int u = 0; u < nf; ++u) {
      if (dead) {
        for (int e = tid; e < D; e += NT) xo[u * D + e] = make_double2(nan, nan);
        continue;
      }
      const double2* yt = fr + (kTile - 1 - u + a.delay) * D;
      const double2* yc = fr + (kTile - 1 - u) * D;
      // ---- A
      for (int e = a_row; e < Me; e += a_step) {
        double ar = 0.0, ai = 0.0;
        if (e < M) {
          const int rbase = e * (e + 1) / 2;
          int c = a_sub;  // two loops without a branch inside, so that the reads run ahead
#pragma unroll 4
          for (; c <= e; c += S) {
            const double2 p = L[rbase + c], v = yt[c];
            ar += p.x * v.x - p.y * v.y;
            ai += p.x * v.y + p.y * v.x;
          }
#pragma unroll 4
          for (; c < M; c += S) {  // conj(l_ce) ytilde_c
            const double2 p = L[c * (c + 1) / 2 + e], v = yt[c];
            ar += p.x * v.x + p.y * v.y;
            ai += p.x * v.y - p.y * v.x;
          }
        } else {  // conj(g_cd) ytilde_c
          const int d = e - M;
#pragma unroll 4
          for (int c = a_sub; c < M; c += S) {
            const double2 g = Gs[c * D + d], v = yt[c];
            ar += g.x * v.x + g.y * v.y;
            ai += g.x * v.y - g.y * v.x;
          }
        }
        for (int o = S >> 1; o > 0; o >>= 1) {
          ar += __shfl_xor(ar, o, 64);
          ai += __shfl_xor(ai, o, 64);
        }
        if (a_sub == 0) {
          if (e < M) {
            nv[e] = make_double2(ar, ai);
          } else {
            const double2 v = yc[e - M];
            const double2 x = make_double2(v.x - ar, v.y - ai);
            xs[e - M] = x;
            xo[u * D + e - M] = x;
          }
        }
      }
      __syncthreads();
      // ---- B
      double t = 0.0, chk = 0.0;
      if (lane < M) {
        const double2 n = nv[lane], v = yt[lane];
        t = v.x * n.x + v.y * n.y;
      }
      if (lane + 64 < M) {
        const double2 n = nv[lane + 64], v = yt[lane + 64];
        t += v.x * n.x + v.y * n.y;
      }
      if (lane < D) {
        const double2 x = xs[lane];
        chk = isfinite(x.x) && isfinite(x.y) ? 0.0 : 1.0;
      }
      t = wave_sum_xor(t);
      chk = wave_sum_xor(chk);
      const double den = a.alpha * lam[u] + t;
      if (!isfinite(den) || chk != 0.0) {  // the same value in every thread
        dead = true;  // from this frame on
        for (int e = tid; e < D; e += NT) xo[u * D + e] = make_double2(nan, nan);
        __syncthreads();
        continue;
      }
      const double g = den > 0.0 ? 1.0 / den : 0.0;
      // ---- C
      for (int pr = c_pair; pr < NP; pr += c_step) {
        const int r1 = pr, r2 = M - 1 - pr;
        const double2 n1 = nv[r1], n2 = nv[r2];
        const int total = r2 != r1 ? M + 1 : r1 + 1;
#pragma unroll 4
        for (int i = c_sub; i < total; i += S2) {
          const bool first = i <= r1;
          const int r = first ? r1 : r2, c = first ? i : i - r1 - 1;
          const double kx = (first ? n1.x : n2.x) * g, ky = (first ? n1.y : n2.y) * g;
          const int idx = r * (r + 1) / 2 + c;
          const double2 nc = nv[c];
          double2 p = L[idx];  // k conj(n_c)
          p.x = (p.x - (kx * nc.x + ky * nc.y)) * a.inv_alpha;
          p.y = c == r ? 0.0 : (p.y - (ky * nc.x - kx * nc.y)) * a.inv_alpha;
          bad |= !(isfinite(p.x) && isfinite(p.y));
          L[idx] = p;
        }
      }
      if (g_d < D) {
        const double2 x = xs[g_d];
        for (int m = g_m; m < M; m += g_step) {
          const double2 n = nv[m];
          const double kx = n.x * g, ky = n.y * g;
          double2 v = Gs[m * D + g_d];  // k conj(x_d)
          v.x += kx * x.x + ky * x.y;
          v.y += ky * x.x - kx * x.y;
          bad |= !(isfinite(v.x) && isfinite(v.y));
          Gs[m * D + g_d] = v;
        }
      }
      __syncthreads();
    }
    __syncthreads();
    // ---- the tile of x, with the strides and the type of y
    for (int idx = tid; idx < nf * D; idx += NT) {
      const TileAt at = tile_index(y, idx, nf);
      const double2 x = xo[at.u * D + at.d];
      const int64_t i = b * y.sb + at.d * y.sd + (t0 + at.u) * y.st;
      if (y.c128)
        static_cast<double2*>(a.out_x)[i] = x;
      else
        static_cast<float2*>(a.out_x)[i] = make_float2((float)x.x, (float)x.y);
    }
    // ---- the newest H frames move behind the tile: slots [kTile - nf, kTile - nf + H) ->
    // [kTile, kTile + H), upwards, so from the top in chunks that are read before they are written
    const int src = (kTile - nf) * D, n = H * D;
    for (int top = n; top > 0; top -= NT) {
      const int e = top - 1 - tid;
      double2 v = make_double2(0.0, 0.0);
      if (e >= 0) v = fr[src + e];
      __syncthreads();
      if (e >= 0) fr[kTile * D + e] = v;
    }
    __syncthreads();
  }

  // ---- the state
  dead = __syncthreads_or(bad) != 0 || dead;
  double2* Po = a.P + b * M * M;
  for (int e = tid; e < M * M; e += NT) {
    const int r = e / M, c = e - r * M;
    double2 v;
    if (c <= r) {
      v = L[r * (r + 1) / 2 + c];
    } else {
      v = L[c * (c + 1) / 2 + r];
      v.y = -v.y;
    }
    Po[e] = dead ? make_double2(nan, nan) : v;
  }
  for (int e = tid; e < M * D; e += NT)
    a.G[b * M * D + e] = dead ? make_double2(nan, nan) : Gs[e];
  for (int e = tid; e < H * D; e += NT) {
    const int d = e / H, i = e - d * H;
    a.hist[(b * D + d) * H + i] = fr[(kTile + H - 1 - i) * D + d];
  }
  if (tid == 0) {
    a.seen[b] = seen + T;
    a.status[b] = dead ? (int32_t)PBBSS_ST_NONFINITE : 0;
  }
}

}  // namespace

int launch_wpe_online(const WpeFrames& y, int64_t B, int taps, int delay, double alpha,
                      const WpeOnlineState& st, void* out_x, int32_t* out_status, hipStream_t s) {
  const size_t lds = wpe_online_lds(y.D, taps, delay);
  const OnlineArgs a{taps, delay, alpha, 1.0 / alpha, st.power,
                     reinterpret_cast<double2*>(st.inv_cov),
                     reinterpret_cast<double2*>(st.filter_taps),
                     reinterpret_cast<double2*>(st.history), st.frames_seen, out_x, out_status};
  auto* kfn = wpe_online_kernel;
  if (!raise_lds_attribute(kfn, lds)) return PBBSS_ERR_LDS_CAPACITY;
  hipLaunchKernelGGL(kfn, dim3((unsigned)B), dim3(NT), lds, s, y, a);
  return hipGetLastError() == hipSuccess ? PBBSS_OK : PBBSS_ERR_HIP;
}

}  // namespace pbbss
