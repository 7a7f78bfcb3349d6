// Host-side entry points of the oracle-mask kernels (masks.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "pbbss.h"

namespace pbbss {

constexpr int kMaskMaxK = 9;        // sources a lane keeps in registers
constexpr int kMaskMaxD = 34;       // sensors pooled per TF point
constexpr int kMaskMaxQ = 8;        // thresholds of one selection sweep
constexpr int kMaskSmallRow = 2048; // longest row of the one-launch selection (values in LDS)

// what the selection looks for in every row, per target j < J
struct MaskTargets {
  int J;
  int lorenz;                    // 1: J == 1, the Lorenz crossing at `fraction`
  double fraction;
  long long rank[kMaskMaxQ];     // quantile: 0-based rank of the lower order statistic
  double gamma[kMaskMaxQ];       //           interpolation weight towards the next one
  int negative[kMaskMaxQ];       //           1: mask = value < threshold, 0: value > threshold
  double high, low;              // mask values of a true / false decision
};

// pointwise masks: one launch.  `table` (3, table_len) is the per-frequency table of the biased
// binary mask, null otherwise.
int launch_mask_pointwise(const void* x, int x_is_c128, int mode, const pbbss_mask_geom& g,
                          double eps, const double* table, int64_t table_len, void* out,
                          hipStream_t s);

// bytes launch_mask_threshold carves from `work` (0 for rows of the one-launch path)
size_t mask_threshold_work_bytes(const pbbss_mask_geom& g, const MaskTargets& t);

// threshold masks (Lorenz / quantile): out in the caller's layout, status (rows) int32
int launch_mask_threshold(const void* x, int x_is_c128, const pbbss_mask_geom& g,
                          const MaskTargets& t, void* work, void* out, int out_is_f64,
                          int32_t* status, hipStream_t s);

}  // namespace pbbss
