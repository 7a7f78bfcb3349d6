// Host-callable launchers of the complex circular-symmetric Gaussian kernels (ccsg.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "pbbss.h"

namespace pbbss {
// The shape plan of both kernels, in one place (pb_bss_amd/engine.py mirrors it as CCSG_* and
// ccsg_class_tile for the Python layer and the tests).
constexpr int kCcsgMaxD = 34;
// log-pdf instantiations: the forward sweep is unrolled for the smallest of these that holds D
constexpr int kCcsgSweepD[] = {4, 8, 16, 34};
// frames per workgroup of both kernels: a log-pdf frame tile and the span of frames whose outer
// products one workgroup of the fit sums (longer rows are split over workgroups)
constexpr int ccsg_frames(int D) { return D <= 8 ? 256 : 128; }
// classes whose Cholesky factors (log-pdf) or saliencies (fit) are in LDS at a time
constexpr int kCcsgMaxClassTile = 8;
constexpr size_t kCcsgLds = 160 * 1024;  // LDS of a gfx950 workgroup

// bytes of the staged frames: rows of D complex128 padded to an odd count of 16-byte slots
constexpr size_t ccsg_frame_lds(int D) { return (size_t)ccsg_frames(D) * (size_t)(D | 1) * 16; }
// LDS of one class of the log-pdf kernel: the factor, its reciprocal diagonal, offset and flag
constexpr size_t ccsg_class_lds(int D) { return (size_t)D * D * 16 + (size_t)D * 8 + 16; }
constexpr int ccsg_class_tile(int D) {
  const size_t fit = (kCcsgLds - ccsg_frame_lds(D)) / ccsg_class_lds(D);
  return fit < (size_t)kCcsgMaxClassTile ? (int)fit : kCcsgMaxClassTile;
}

// complex128 partial sums of launch_ccsg_fit (one (D (D + 1) / 2 + 1)-vector per span and class)
size_t ccsg_fit_partials(int64_t B, int64_t N, int D, int K);

// ComplexCircularSymmetricGaussianTrainer._fit (complex_circular_symmetric_gaussian.py:94-116)
int launch_ccsg_fit(const void* y, int y_is_c128, int64_t B, int64_t N, int D, int K,
                    const void* saliency, int saliency_is_f64, double floor, double* part,
                    double* out_cov, hipStream_t s);
// ComplexCircularSymmetricGaussian.log_pdf (:26-48)
int launch_ccsg_log_pdf(const void* y, int y_is_c128, int64_t B, int64_t N, int D, int K,
                        const double* cov, double* out_lp, double* out_log_det,
                        int32_t* out_status, hipStream_t s);
}  // namespace pbbss
