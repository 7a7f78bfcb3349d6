// Griffin-Lim / MISI phase reconstruction (griffin_lim.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pbbss.h"

namespace pbbss {

constexpr int kMisiMaxSources = 8;  // one thread of the overlap-add holds a mixture's sums

struct GriffinLimProblem {
  const void* X;           // (B, K, T, size/2+1) complex64 / complex128: the magnitudes
  int x_is_c128;
  const double* y;         // (B, n) mixtures: MISI; nullptr: Griffin-Lim
  int64_t B;
  int K, T, size, shift, fade;
  const double* analysis_window;   // (size)
  const double* synthesis_window;  // (size) biorthogonal
  int iterations;
  double* x_hat;           // (B, K, n) in: current estimate, out: after the iterations
  void* X_dash_dash;       // (B, K, T, size/2+1) complex128 of the last iteration, or nullptr
  void* X_dash;            // both or neither
  int64_t n;
};

// bytes of device scratch run_griffin_lim needs: the frames and (MISI) the corrected rows
size_t griffin_lim_scratch_bytes(const GriffinLimProblem& p);

// `iterations` times [projection, overlap-add] on `s` (MISI: the correction of the first guess in
// front), ordinary launches only.  scratch: griffin_lim_scratch_bytes(p) bytes.
int run_griffin_lim(const GriffinLimProblem& p, void* scratch, size_t lds_limit, hipStream_t s);

}  // namespace pbbss
