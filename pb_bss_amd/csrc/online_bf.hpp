// Host-callable launcher of the frame-recursive mask-driven MVDR kernel (online_bf.hip).
#pragma once
#include "wpe.hpp"

namespace pbbss {
// The shape plan of the kernel (pb_bss_amd/engine.py mirrors it as ONLINE_BF_*).
constexpr int kOnlineBfMaxD = 16;             // sensors
constexpr int kOnlineBfTile = 32;             // frames staged, and output frames written, at a time
constexpr int kOnlineBfD[] = {4, 8, 16};      // instantiations: the smallest bound that holds D
// One wavefront per problem and no workgroup barrier anywhere; four problems share a workgroup
// only so that one workgroup fills the four SIMDs of a compute unit.
constexpr int kOnlineBfWaves = 4;

struct OnlineBfArgs {
  const void *target_mask, *noise_mask;  // (B, T) float32 / float64
  int mask_f64;
  double alpha;
  int ref;
  double* target_psd;    // (B, D, D) complex128, in / out
  double* noise_inv;     // (B, D, D) complex128, in / out
  int64_t* frames_seen;  // (B), in / out
  void* out_x;           // (B, T), the type of the frames
  double* out_w;         // (T, B, D) complex128, or null
  int32_t* status;       // (B)
};

// T frames of the recursion for B problems
int launch_online_mvdr(const WpeFrames& y, int64_t B, const OnlineBfArgs& a, hipStream_t s);
}  // namespace pbbss
