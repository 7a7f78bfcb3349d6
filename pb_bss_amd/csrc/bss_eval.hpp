// Host-side entry points of the BSS-Eval kernels (bss_eval.hip): SDR / SIR / SAR of time signals
// by the time-invariant-filter least-squares decomposition of BSS Eval 3.0.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "carver.hpp"
#include "eval.hpp"

namespace pbbss {

constexpr int kBssCorrSpan = 2048;  // samples one correlation workgroup owns (plus an L - 1 halo)
constexpr int kBssSynSpan = 1024;   // output samples one synthesis workgroup owns
constexpr int kBssThreads = 256;
constexpr int kBssMaxFilter = 512;  // filter length of mir_eval and of the reference's K+1 variant
constexpr int kBssMaxSources = 8;   // OutputMetrics.check_inputs; 8! candidate selections
constexpr int kBssPanel = 32;       // panel width of the blocked Cholesky factorisation
constexpr int kBssSolveRhs = 4;     // right-hand sides one triangular-solve workgroup carries
constexpr int64_t kBssMaxGroup = 32768;            // items of one launch set (grid.z)
constexpr size_t kBssGroupBytes = size_t(1) << 30; // workspace one group of items may take

// One call: B items of K reference rows and Ke estimation rows of N samples (element strides;
// ref_batch == 0: the same references for every item, correlated and factorised once).
struct BssProblem {
  const void* ref;
  const void* est;
  int64_t B, N;
  int64_t ref_batch, ref_row, est_batch, est_row;
  int K, Ke, L, is_f64, permute;
};

// Filters handed in by the caller in place of the device solve (the host fallback of items whose
// Gram matrix the Cholesky factorisation refuses): all (B, Ke, K L), single (B, Ke, K, L).
struct BssFilters {
  const double* all;
  const double* single;
};

struct BssOutputs {
  double *sdr, *sir, *sar;  // (B, K)
  int64_t* selection;       // (B, K)
  double* tables;           // (B, 3, Ke, K) or null
  int32_t* status;          // (B)
};

// the pieces of the workspace of one group of items
struct BssWork {
  double *p_rr, *rr, *p_re, *re, *mats, *c_all, *c_single, *p_syn;
  int32_t* fail;
};

inline int bss_pad(int n) { return (n + kBssPanel - 1) / kBssPanel * kBssPanel; }
inline int64_t bss_corr_chunks(int64_t N) { return (N + kBssCorrSpan - 1) / kBssCorrSpan; }
inline int64_t bss_syn_chunks(int64_t N, int L) { return (N + L - 1 + kBssSynSpan - 1) / kBssSynSpan; }

// items one launch set covers (as many as fit kBssGroupBytes, one at least), the take() calls of
// the workspace of that many items, and their bytes
int64_t bss_group_items(const BssProblem& p);
void bss_carve(Carver& c, const BssProblem& p, int64_t items, BssWork& w);
size_t bss_group_work(const BssProblem& p, int64_t items);

// the whole metric for items [0, B) in groups of `group`; work: carved for `group` items.
// filters == nullptr: correlate, factorise and solve on the device.  phase_ms (or null): four
// floats the device time of the phases is added to; the call then waits for every group.
int launch_bss_eval(const BssProblem& p, const BssFilters* filters, const BssWork& work,
                    int64_t group, const BssOutputs& out, float* phase_ms, hipStream_t s);
// the normal equations alone: G (Bref, K L, K L) with Bref = 1 for shared references, D (B, Ke, K L)
int launch_bss_system(const BssProblem& p, const BssWork& work, int64_t group, double* out_G,
                      double* out_D, hipStream_t s);

}  // namespace pbbss
