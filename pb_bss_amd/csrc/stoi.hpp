// Host-side entry points of the polyphase resampler and the STOI kernels (stoi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "carver.hpp"
#include "pbbss.h"

namespace pbbss {

constexpr int kStoiFrame = 256;                       // samples of a frame at 10 kHz
constexpr int kStoiHop = 128;
constexpr int kStoiBands = 15;                        // third-octave bands from 150 Hz
constexpr int kStoiSegment = 30;                      // frames of one correlation segment
constexpr int kStoiSegThreads = 256;                  // (segment, band) items of one workgroup
constexpr int64_t kStoiMaxLength = int64_t(1) << 24;  // samples of a row (int32 indices)
constexpr int64_t kStoiMaxRows = 65535;               // rows are a grid y extent

// frames of a row before the removal: range(0, N10 - 256, 128)
inline int64_t stoi_frames(int64_t N10) {
  return N10 > kStoiFrame ? (N10 - kStoiFrame + kStoiHop - 1) / kStoiHop : 0;
}
// upper bound of a row's STFT frames T = kept - 1, and of its workgroups of segment items
inline int64_t stoi_max_stft_frames(int64_t N10) {
  const int64_t F = stoi_frames(N10);
  return F > 0 ? F - 1 : 0;
}
inline int64_t stoi_max_partials(int64_t N10) {
  const int64_t J = stoi_max_stft_frames(N10) - (kStoiSegment - 1);
  return J > 0 ? (J * kStoiBands + kStoiSegThreads - 1) / kStoiSegThreads : 0;
}
inline int64_t resample_length(int64_t N, int up, int down) { return (N * up + down - 1) / down; }

// rows = outer * inner pairs; row (o, i) of x starts at x + o x_outer + i x_inner doubles (y
// alike), a stride may be 0
struct StoiRows {
  const double* x;
  const double* y;
  int64_t outer, inner, N10;
  int64_t x_outer, x_inner, y_outer, y_inner;
};

struct StoiWork {
  double* energy;   // (rows, F) frame energies of x in dB
  int32_t* src;     // (rows, F) source frame of every kept frame
  int32_t* kept;    // (rows) kept frames
  double* tob;      // (rows, 2, Tmax, 15) third-octave band magnitudes of x and y
  double* partial;  // (rows, Pmax) sums of the workgroups of the segment kernel
};

inline void stoi_workspace(Carver& c, int64_t rows, int64_t N10, StoiWork* w) {
  const int64_t F = stoi_frames(N10);
  w->energy = c.take<double>((size_t)(rows * F));
  w->src = c.take<int32_t>((size_t)(rows * F));
  w->kept = c.take<int32_t>((size_t)rows);
  w->tob = c.take<double>((size_t)(rows * 2 * stoi_max_stft_frames(N10) * kStoiBands));
  w->partial = c.take<double>((size_t)(rows * stoi_max_partials(N10)));
}

// window: 2 half + 1 taps; out (rows, resample_length(N, up, down))
int launch_resample_poly(const void* x, int is_f64, int64_t rows, int64_t N, int up, int down,
                         const double* window, int half, double* out, hipStream_t s);
// out (rows); out_frames (rows, 2) or null
int launch_stoi(const StoiRows& g, const StoiWork& w, double* out, int32_t* out_frames,
                hipStream_t s);

}  // namespace pbbss
