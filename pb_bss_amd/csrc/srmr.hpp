// Host-side entry points of the gammatone filterbank and the SRMR kernels (srmr.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "pbbss.h"

namespace pbbss {

constexpr int kBiquadChunk = 64;                 // samples of the chunk one lane owns
constexpr int kBiquadTile = 64 * kBiquadChunk;   // samples one wavefront filters per lane-group
constexpr int kGammatoneStages = 4;              // cascaded biquads of one cochlear channel
constexpr int kSrmrModFilters = 8;               // modulation filters of every envelope
constexpr int kSrmrMaxChannels = 64;             // cochlear channels of one call
constexpr int64_t kSrmrMaxLength = int64_t(1) << 24;  // samples of a row (int32 indices, scans)
constexpr int kSrmrMinSampleRate = 1000;         // below, the frame length int(rate/1000)*256 is 0
constexpr int kBiquadCoefs = 5;                  // b0 b1 b2 a1 a2 (a0 = 1)

inline int srmr_frame_hop(int sample_rate) { return (sample_rate / 1000) * 64; }
inline int srmr_frame_length(int sample_rate) { return (sample_rate / 1000) * 256; }

// right_ws: rows * N int32 (nearest flagged index at or after every sample)
int launch_srmr_vad(const void* x, int is_f64, int64_t rows, int64_t N, int sample_rate,
                    int32_t* right_ws, double* out, int32_t* out_lengths, hipStream_t s);
int launch_gammatone(const void* x, int is_f64, int64_t rows, int64_t N, const int32_t* lengths,
                     int n, const double* coef, double* out, hipStream_t s);
// weights: rows * N doubles (the per-sample frame weight W[t] of every row)
int launch_srmr_energies(const void* analytic, int64_t rows, int64_t N, const int32_t* lengths,
                         int n, int sample_rate, const double* coef, double* weights,
                         double* out_means, hipStream_t s);
int launch_srmr_score(const double* means, int64_t rows, int n, const double* erbs,
                      const double* cutoffs, double* out, hipStream_t s);

}  // namespace pbbss
