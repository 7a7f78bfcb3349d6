// The lane grid of the wave-per-problem recursive kernels (online_bf.hip, online_cacgmm.hip).
//
// A D x D Hermitian matrix, D <= DB, lives in registers as a FULL matrix on the 64 lanes of the
// wavefront that serves the problem: lane l owns row l / LPR and the columns l % LPR + e LPR,
// e < E, with (LPR, E) = (4, 1), (8, 1), (4, 4) for the sensor bounds 4, 8, 16.  Every lane
// computes the element of the LOWER triangle that it owns or mirrors, (max(r, c), min(r, c)), with
// the same instructions on the same values as its mirror lane, and stores the conjugate when it
// sits above the diagonal.  The upper triangle therefore is the conjugate mirror to the bit, as
// the definition demands, and no transpose ever crosses the lanes.  Rows and columns beyond D hold
// zeros, which every update maps to zeros.  Sums over a row are fixed DPP trees, so the order of
// the additions never depends on blocking or on the batch.
//
// Frames lie in the wavefront's slice of LDS as [frame][DB] with zeros beyond D (frame_tile.hpp
// stages them there).
#pragma once
#include "pbbss_dev.hpp"

namespace pbbss {

// ---- wave64 building blocks beside those of pbbss_dev.hpp (kept out of that header: it is one
// of the EM kernels' sources whose hash the committed profiles carry, tools/bench_blocks.py)

// K sums over the 64 lanes, on every lane: the tree of wave_sum, stage by stage for all K, so
// that the K chains of exchanges and additions interleave
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
// all-reduce over each aligned group of 8 lanes: the first three stages of wave_allreduce
template <typename Op>
__device__ __forceinline__ double lanes8_allreduce(double v, Op op) {
  v = op(v, dpp_mov_f64<kDppQuadXor1>(v));
  v = op(v, dpp_mov_f64<kDppQuadXor2>(v));
  return op(v, dpp_mov_f64<kDppRowHalfMirror>(v));
}
__device__ __forceinline__ double lanes8_sum(double v) {
  return lanes8_allreduce(v, [](double x, double y) { return x + y; });
}
__device__ __forceinline__ double lanes8_max(double v) {
  return lanes8_allreduce(v, [](double x, double y) { return fmax(x, y); });
}
// the value of lane `src` (a compile-time constant) on every lane, through scalar registers
__device__ __forceinline__ double lane_const(double v, int src) {
  F64Bits s, r;
  s.d = v;
  r.i[0] = __builtin_amdgcn_readlane(s.i[0], src);
  r.i[1] = __builtin_amdgcn_readlane(s.i[1], src);
  return r.d;
}

// sums over the LPR lanes of a row of the lane grid, on every lane of the row, for K values
// (a[k], b[k]), stage by stage
template <int LPR, int K>
__device__ __forceinline__ void row_sums(double* a, double* b) {
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

template <int DB>
struct LaneGrid {
  static constexpr int LPR = DB == 8 ? 8 : 4;  // lanes per row
  static constexpr int E = DB / LPR;           // columns per lane
  static_assert(LPR * DB <= kWave && E * LPR == DB);
  int r, cl, rr;  // row, first column, and the row clamped to one that exists
  bool rowok, act[E], lower[E], diag[E];

  __device__ __forceinline__ LaneGrid(int lane, int D) {
    r = lane / LPR;
    cl = lane - r * LPR;
    rowok = r < D;
    rr = rowok ? r : 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int c = cl + e * LPR;
      act[e] = rowok && c < D;
      lower[e] = r >= c;
      diag[e] = r == c;
    }
  }

  // the lower triangle and the real diagonal of M are read
  __device__ __forceinline__ void load_hermitian(const double2* M, int D, double2 (&m)[E]) const {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int c = cl + e * LPR;
      double2 v = make_double2(0.0, 0.0);
      if (act[e]) {
        v = M[lower[e] ? r * D + c : c * D + r];
        if (!lower[e]) v.y = -v.y;
        if (diag[e]) v.y = 0.0;
      }
      m[e] = v;
    }
  }
  // the whole matrix, Hermitian to the bit; NaN when the recursion has stopped
  __device__ __forceinline__ void store_hermitian(double2* M, int D, const double2 (&m)[E],
                                                  bool dead) const {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (act[e]) M[r * D + cl + e * LPR] = dead ? make_double2(nan, nan) : m[e];
  }

  // y_r and the y_c of this lane's columns of tile frame u
  __device__ __forceinline__ void read_frame(const double2* fr, int u, double2& yr,
                                             double2 (&yc)[E]) const {
    const double2 v = fr[u * DB + rr];
    yr = rowok ? v : make_double2(0.0, 0.0);
#pragma unroll
    for (int e = 0; e < E; ++e) yc[e] = fr[u * DB + cl + e * LPR];
  }

  // P <- (P - (coef n) n^H) scale with n_r = (nr, ni) on every lane of row r: n_c comes from the
  // lanes of row c (the one LDS-crossbar hop on the chain P -> P)
  __device__ __forceinline__ void downdate(double2 (&P)[E], double nr, double ni, double coef,
                                           double scale) const {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int src = (cl + e * LPR) * LPR;  // a lane of row c
      const double cr = lane_get(nr, src), ci = lane_get(ni, src);
      const double Rr = lower[e] ? nr : cr, Ri = lower[e] ? ni : ci;
      const double Cr = lower[e] ? cr : nr, Ci = lower[e] ? ci : ni;
      const double kx = Rr * coef, ky = Ri * coef;
      double2 p = P[e];
      double ly = lower[e] ? p.y : -p.y;
      p.x = (p.x - (kx * Cr + ky * Ci)) * scale;
      ly = diag[e] ? 0.0 : (ly - (ky * Cr - kx * Ci)) * scale;
      p.y = lower[e] ? ly : -ly;
      P[e] = p;
    }
  }
};

}  // namespace pbbss
