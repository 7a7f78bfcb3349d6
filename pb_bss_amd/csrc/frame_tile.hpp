// Frames read through a WpeFrames view, and the tile staging of the frame-recursive kernels
// (wpe_online.hip, online_bf.hip, online_cacgmm.hip): the next tile of frames waits in registers
// while the frames of this one are worked on, and is handed to LDS at the tile's start, so no
// global load sits on the per-frame chain and a frame is read from global memory once.
#pragma once
#include "wpe.hpp"

namespace pbbss {

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

// A tile of up to kTile frames of at most DB sensors, spread over the NT threads that serve a
// problem.  The array is indexed by unrolled loops only, so it stays in registers.
template <int kTile, int DB, int NT>
struct TilePrefetch {
  static constexpr int kPre = kTile * DB / NT;  // elements of a tile per thread
  static_assert(kPre * NT == kTile * DB);
  double2 pre[kPre];

  static __device__ __forceinline__ int frames(int64_t T, int64_t t0) {
    return (int)(T - t0 < kTile ? T - t0 : kTile);
  }
  // frames t0 .. of problem b -> registers
  __device__ __forceinline__ void fetch(const WpeFrames& y, int64_t b, int64_t t0, int tid) {
    const int nf = frames(y.T, t0);
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
      const int idx = tid + NT * i;
      pre[i] = make_double2(0.0, 0.0);
      if (idx < nf * y.D) {
        const TileAt at = tile_index(y, idx, nf);
        pre[i] = load_frame(y, b * y.sb + at.d * y.sd + (t0 + at.u) * y.st);
      }
    }
  }
  // registers -> fr[slot(u, d)], sensor d of tile frame u; t0 and tid as they were fetched
  template <typename Slot>
  __device__ __forceinline__ void stage(const WpeFrames& y, int64_t t0, int tid, double2* fr,
                                        Slot slot) const {
    const int nf = frames(y.T, t0);
#pragma unroll
    for (int i = 0; i < kPre; ++i) {
      const int idx = tid + NT * i;
      if (idx < nf * y.D) {
        const TileAt at = tile_index(y, idx, nf);
        fr[slot(at.u, at.d)] = pre[i];
      }
    }
  }
};

}  // namespace pbbss
