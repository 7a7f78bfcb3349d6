// Host-callable launcher of the frame-recursive WPE kernel (wpe_online.hip).
#pragma once
#include "wpe.hpp"

namespace pbbss {
// The shape plan of the kernel (pb_bss_amd/engine.py mirrors it as WPE_ONLINE_*).
constexpr int kWpeOnlineTile = 32;        // frames staged, and output frames written, at a time
constexpr int kWpeOnlineMaxRing = 2048;   // D * (taps + delay): the frames kept behind the stream
// One workgroup of four wavefronts per problem whatever D * taps is: the lanes per row follow M, so
// a small problem does not leave the workgroup idle (a one-wavefront variant was measured and
// loses: DESIGN 4.19).
constexpr int kWpeOnlineThreads = 256;
static_assert(kWpeOnlineTile * kWpeMaxD % kWpeOnlineThreads == 0);

// LDS (bytes): packed lower triangle of P | G [M][D] | frames [taps + delay + tile][D], newest
// first | output tile [tile][D] | n [M] | x [16] complex128 | lambda [tile] float64
constexpr size_t wpe_online_lds(int D, int taps, int delay) {
  return ((size_t)D * taps * (D * taps + 1) / 2 + (size_t)D * taps * D +
          (size_t)(taps + delay + kWpeOnlineTile) * D + (size_t)kWpeOnlineTile * D +
          (size_t)D * taps + kWpeMaxD) * 16 + kWpeOnlineTile * 8;
}
static_assert(wpe_online_lds(16, 6, kWpeOnlineMaxRing / 16 - 6) <= kWpeLds &&
              wpe_online_lds(8, 12, kWpeOnlineMaxRing / 8 - 12) <= kWpeLds &&
              wpe_online_lds(1, 96, kWpeOnlineMaxRing - 96) <= kWpeLds);

struct WpeOnlineState {
  const double* power;   // (B, T) lambda_t, or null: the causal power of the frames themselves
  double* inv_cov;       // (B, M, M) complex128, in / out
  double* filter_taps;   // (B, M, D) complex128, in / out
  double* history;       // (B, D, taps + delay) complex128, newest frame last, in / out
  int64_t* frames_seen;  // (B), in / out
};

// T frames of the recursion for B problems
int launch_wpe_online(const WpeFrames& y, int64_t B, int taps, int delay, double alpha,
                      const WpeOnlineState& st, void* out_x, int32_t* out_status, hipStream_t s);
}  // namespace pbbss
