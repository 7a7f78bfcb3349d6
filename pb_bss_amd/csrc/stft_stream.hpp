// Streaming STFT / inverse STFT launchers (stft_stream.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pbbss.h"

namespace pbbss {

// One call of a forward stream.  Positions are relative to the first sample of the block: the
// history holds the `hist_len` samples in front of it (hist[hist_len + r] for r < 0), the block
// the samples 0 <= r < n.
struct StftStreamArgs {
  const void* x;            // (C, n) float32 / float64 block; never read where n == 0
  int x_is_f64;
  int64_t C, n;
  const double* hist_in;    // (C, hist_len) the samples in front of the block, newest last
  double* hist_out;         // (C, hist_len) the same behind the block; another buffer than hist_in
  int hist_len;             // max(1, window_length - 1)
  int64_t lo;               // positions r < lo lie in front of the stream: zero
  int64_t base;             // position of the first sample of the first frame written
  int m;                    // frames written
  int reset;                // hist_out = 0 (flush) instead of the history behind the block
  int size, shift, wl;
  const double* window;     // (wl) analysis window
  int layout;               // 0: out (C, m, F), 1: out (F, m, C)
  int out_c128;
  void* out;
};

int launch_stft_stream(const StftStreamArgs& a, size_t lds_limit, hipStream_t s);

// One call of an inverse stream: m frames of `rows` rows, read through their strides.
struct IstftStreamArgs {
  const void* X;            // complex64 / complex128, element (row, t, k) at the strides below
  int x_is_c128;
  int64_t rows;
  int m;
  int64_t stride_r, stride_t, stride_f;  // in complex elements
  int size, shift, wl;
  const double* window;     // (wl) synthesis (biorthogonal) window
  double* tail;             // (rows, wl - shift) overlap tail, read and rewritten
  int skip;                 // samples of this call in front of the output (the dropped fade-in)
  double* out;              // (rows, n_out), n_out = m * shift - skip
  int64_t n_out;
};

int launch_istft_stream(const IstftStreamArgs& a, size_t lds_limit, hipStream_t s);

}  // namespace pbbss
