// Host-callable launcher of the frame-recursive cACGMM mask estimator (online_cacgmm.hip).
#pragma once
#include "wpe.hpp"

namespace pbbss {
// The shape plan of the kernel (pb_bss_amd/engine.py mirrors it as ONLINE_CACGMM_*).
constexpr int kOnlineCacgmmMaxD = 16;         // sensors
constexpr int kOnlineCacgmmMaxK = 8;          // classes: one lane of an 8-lane group each
constexpr int kOnlineCacgmmTile = 32;         // frames staged, and output frames written, at a time
constexpr int kOnlineCacgmmD[] = {4, 8, 16};  // instantiations: the smallest bound that holds D
// One wavefront per problem and no workgroup barrier anywhere; four problems share a workgroup
// only so that one workgroup fills the four SIMDs of a compute unit.
constexpr int kOnlineCacgmmWaves = 4;

struct OnlineCacgmmArgs {
  int K;
  double alpha, affiliation_eps;
  int update_weight;
  double* precision;        // (B, K, D, D) complex128, in / out
  double* log_determinant;  // (B, K), in / out
  double* count;            // (B, K), in / out
  double* weight;           // (B, K), in / out
  int64_t* frames_seen;     // (B), in / out
  double* out_affiliation;  // (B, K, T)
  double* out_q;            // (B, K, T), or null
  int32_t* status;          // (B)
};

// T frames of the recursion for B problems
int launch_online_cacgmm(const WpeFrames& y, int64_t B, const OnlineCacgmmArgs& a, hipStream_t s);
}  // namespace pbbss
