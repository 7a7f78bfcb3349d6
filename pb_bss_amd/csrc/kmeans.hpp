// Host-side entry points of the k-means kernels (kmeans.hip): Lloyd sweeps with a device-side
// stop, greedy k-means++ seeding, label / one-hot prediction.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "pbbss.h"

namespace pbbss {

constexpr int kKmeansThreads = 256;  // lanes of every k-means workgroup
constexpr int kKmeansMaxK = 64;      // EMBED_MAX_CLASSES
constexpr int kKmeansMaxE = 256;     // kEmbedMaxE
constexpr int kKmeansFastK = 8;      // class sums in registers up to here ...
constexpr int kKmeansFastE = 64;     // ... and this many columns; beyond: class sums in LDS
constexpr int kKmeansScanRows = 1024;  // rows of one chunk of the seeding's prefix sum
constexpr int kKmeansMaxTrials = 8;    // 2 + int(log 64) = 6 local trials at most
// Workgroups one sweep aims at.  A constant, not the device's compute-unit count: the chunking
// fixes the order of the partial sums, so results do not depend on the device.
constexpr int kKmeansTargetWorkgroups = 512;

// state of one problem b of a fit
constexpr int kKmeansRunning = 0;  // Lloyd iterations go on
constexpr int kKmeansRelabel = 1;  // stopped by tol / max_iter: the last sweep assigns labels anew
constexpr int kKmeansInvalid = 2;  // fewer selected rows than classes
constexpr int kKmeansStrict = 3;   // no label changed: the last sweep keeps the labels

// How one problem's rows are cut up: C chunks of L rows (tiles of R rows) per problem.
struct KmeansGeom {
  int64_t B, N, C, L, scan_chunks;
  int E, K, is_f64;
  int KT;      // class accumulators in registers (2, 3, 4 or 8), 0: in LDS
  int R, S;    // rows of a tile; row slots of the accumulation
  size_t lds;  // dynamic LDS of the sweep kernel
};
// false: outside the served range (1 <= K <= 64, 1 <= E <= 256) or too large for one grid
bool kmeans_geom(int64_t B, int64_t N, int E, int K, int is_f64, KmeansGeom* g);
inline size_t kmeans_part_len(const KmeansGeom& g) { return (size_t)g.K * (g.E + 1) + 2; }

struct KmeansWork {
  double* part;     // (B, C, K (E + 1) + 2) chunk partials: class sums | counts, inertia, changed
  double* tot;      // (B, K, E + 1) the partials added up
  double* mind;     // (B, N) squared distance of a row to its centre
  double* mean;     // (B, E + 1) column means | selected rows
  double* tol_abs;  // (B) tol * mean_e var_n x
  int32_t* state;   // (B)
  int32_t* flags;   // [0] problems still running, [1] a problem with fewer rows than classes
};

struct KmeansSeedWork {
  double* closest;  // (B, N)
  double* csum;     // (B, scan_chunks)
  double* cpart;    // (B, scan_chunks, kKmeansMaxTrials)
  int32_t* cand;    // (B, kKmeansMaxTrials)
  int32_t* chosen;  // (B)
};

// PBBSS_OK, PBBSS_ERR_HIP, or PBBSS_ERR_INVALID_ARG when a problem selects fewer than K rows
int run_kmeans_fit(const KmeansGeom& g, const KmeansWork& w, const void* y, const uint8_t* sal,
                   int max_iter, double tol, int block, double* centers, int32_t* labels,
                   double* inertia, int32_t* n_iter, hipStream_t s);
int run_kmeans_predict(const KmeansGeom& g, const KmeansWork& w, const void* y,
                       const double* centers, int32_t* labels, void* one_hot, double* inertia,
                       hipStream_t s);
int run_kmeans_plusplus(const KmeansGeom& g, const KmeansSeedWork& w, const void* y,
                        const uint8_t* sal, int trials, const double* randoms, int32_t* indices,
                        double* centers, hipStream_t s);

}  // namespace pbbss
