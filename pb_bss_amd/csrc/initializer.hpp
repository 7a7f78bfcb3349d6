// Host-side entry point of the deflation-seed kernels (initializer.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pbbss {

struct DeflationArgs {
  const void* y;         // (B, F, T, D) complex64 / complex128
  int y_is_c128;
  int64_t B;
  int F, T, D, K;
  const double* sal_in;  // (B, F, T) caller's saliencies, or null: ||y||
  double* sal_state;     // (B, F, T) running saliencies between launches
  int permutation_free;
  int neighbors;
  double eps;
  int r0, r1;            // rounds [r0, r1) of the K - 1 deflation rounds
  int finalize;          // last class, flooring and class normalisation
  double* out;           // (B, K, F, T)
  int32_t* out_peak;     // (B, K - 1, F) clipped peak frame of each round, or null
  // workspace
  double* colmean;       // (B, T): mean saliency over the bins (permutation-free form)
  double* psd;           // D > 8: (B F, D, D) complex, local PSD of the round
  double* eigval;        //        (B F, D)
  double* eigvec;        //        (B F, D, D) complex
  int32_t* eigst;        //        (B F)
};

// bytes launch_deflation_seed carves from `work`: the pointers of the workspace block, and the
// saliency state where the call needs one and the caller gave none
size_t deflation_work_bytes(const DeflationArgs& a, int init, size_t lds_limit);

// init: start from a.sal_in / ||y|| (else from a.sal_state, which an earlier call left)
int launch_deflation_seed(DeflationArgs a, int init, void* work, size_t lds_limit, hipStream_t s);

}  // namespace pbbss
