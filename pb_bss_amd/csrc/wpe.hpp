// Host-callable launchers of the WPE dereverberation kernels (wpe.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "pbbss.h"

namespace pbbss {
// The shape plan of the kernels, in one place (pb_bss_amd/engine.py mirrors it as WPE_* for the
// Python layer and the tests).
constexpr int kWpeMaxD = 16;   // sensors
constexpr int kWpeMaxM = 96;   // stacked length D * taps (8 sensors x 12 taps, 16 x 6)
constexpr int kWpeTile = 16;   // edge of a v_mfma_f64_16x16x4_f64 tile
// frames whose outer products one workgroup of the correlation kernel sums; longer rows are split
// over workgroups and the span sums are added in ascending order
constexpr int kWpeSpan = 128;
// tile rows of the extended Gram matrix (M + D <= 112 rows) and of its lower block triangle
constexpr int kWpeMaxBlocks = (kWpeMaxM + kWpeMaxD + kWpeTile - 1) / kWpeTile;
// correlation instantiations: accumulator tiles per wavefront (four wavefronts share the triangle)
constexpr int kWpeCorrTiles[] = {2, 4, 7};
static_assert(kWpeCorrTiles[2] * 4 >= kWpeMaxBlocks * (kWpeMaxBlocks + 1) / 2);
constexpr int kWpeApplyFrames = 256;        // frames per workgroup of the filter kernel
constexpr int kWpeApplyD[] = {4, 8, 16};    // filter instantiations: the smallest bound that holds D
constexpr size_t kWpeLds = 160 * 1024;      // LDS of a gfx950 workgroup
constexpr size_t kWpeWorkspaceCap = (size_t)512 << 20;  // span sums of one chunk of problems

constexpr int wpe_blocks(int D, int taps) { return (D * taps + D + kWpeTile - 1) / kWpeTile; }
constexpr int wpe_tiles(int D, int taps) { return wpe_blocks(D, taps) * (wpe_blocks(D, taps) + 1) / 2; }
constexpr int64_t wpe_spans(int64_t T) { return (T + kWpeSpan - 1) / kWpeSpan; }
// LDS of the three kernels (bytes)
constexpr size_t wpe_corr_lds(int D, int taps) {
  return ((size_t)D * (kWpeSpan + 1) + (size_t)D * ((kWpeSpan + taps - 1) | 1)) * 16 + kWpeSpan * 8;
}
constexpr size_t wpe_solve_lds(int D, int taps) {
  return ((size_t)D * taps * (D * taps + 1) / 2 + (size_t)D * taps * D) * 16 + (size_t)D * taps * 8;
}
constexpr size_t wpe_apply_lds(int D, int taps) {
  return ((size_t)D * taps * D + (size_t)D * ((kWpeApplyFrames + taps - 1) | 1)) * 16;
}
static_assert(wpe_solve_lds(8, 12) <= kWpeLds && wpe_solve_lds(16, 6) <= kWpeLds &&
              wpe_corr_lds(16, 6) <= kWpeLds && wpe_corr_lds(1, 96) <= kWpeLds &&
              wpe_apply_lds(16, 6) <= kWpeLds && wpe_apply_lds(1, 96) <= kWpeLds);

// A strided (B, D, T) view of complex frames: element (b, d, t) at b * sb + d * sd + t * st
// (in complex elements); c128 = interleaved float64, else float32.
struct WpeFrames {
  const void* p;
  int c128;
  int64_t T, sb, sd, st;
  int D;
};

// device floats of one chunk of problems
struct WpeWork {
  double *raw, *power, *inv, *pmax;  // (B, T) unsmoothed, (B, T), (B, T), (B)
  double* part;                // (B, spans, tiles, 256) complex128
  double *R, *P, *G;           // (B, M, M), (B, M, D), (B, M, D) complex128
};

// get_power + get_power_inverse: power (mean over the sensors, smoothed over psd_context frames
// on either side; -1 = all frames) and 1 / max(power, 1e-10 max_t power); either output may be
// null.  `raw`: a (B, T) power that is already there (then `y` is not read).
int launch_wpe_inverse_power(const WpeFrames& y, const double* raw, int64_t B, int64_t psd_context,
                             double* raw_work, double* out_power, double* out_inv, double* out_pmax,
                             hipStream_t s);
// get_correlations: R (B, M, M) and P (B, M, D) from the frames and the weights
int launch_wpe_correlations(const WpeFrames& y, int64_t B, const double* inv, int taps, int delay,
                            int valid, double* part, double* out_R, double* out_P, hipStream_t s);
// get_filter_matrix: G = R^-1 P by Cholesky; a problem whose pmax is 0 gets G = 0
int launch_wpe_solve(const double* R, const double* P, const double* pmax, int64_t B, int D,
                     int taps, double* out_G, int32_t* out_status, hipStream_t s);
// perform_filter_operation: x = y - G^H ytilde (out_x null: only the power of x is written)
int launch_wpe_apply(const WpeFrames& y, int64_t B, const double* G, int taps, int delay,
                     void* out_x, double* out_power, hipStream_t s);
}  // namespace pbbss
