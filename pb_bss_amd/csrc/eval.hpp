// Host-side entry points of the evaluation-metric kernels (eval.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "pbbss.h"

namespace pbbss {

constexpr int kEvalSpan = 4096;    // samples of every row one workgroup owns
constexpr int kEvalThreads = 256;  // lanes of a streaming workgroup
// workgroups of one streaming launch: fewer than 2^32 lanes in the grid
constexpr int64_t kEvalMaxWorkgroups = (int64_t(1) << 24) - 1;
constexpr int kEvalMaxRows = 8;    // rows of each si_sdr argument a lane keeps in registers
constexpr int kSxrMaxTargets = 8;  // output_sxr: 8! = 40 320 candidate selections at most
constexpr int kSxrMaxSources = 9;  // input_sxr: the reference asserts K < 10
constexpr int kSxrMaxSensors = 29; // input_sxr: the reference asserts D < 30

// The rows of one streaming pass: B items of Kr reference and Ke estimation rows of N real
// samples each (element strides; a complex row is passed as 2 N reals).
struct EvalRows {
  const void* ref;
  const void* est;
  int64_t B, N;
  int64_t ref_batch, ref_row, est_batch, est_row;
  int Kr, Ke, is_f64;
};

inline int64_t eval_chunks(int64_t N) { return N < 1 ? 1 : (N + kEvalSpan - 1) / kEvalSpan; }
inline bool eval_is_complex(int dtype) { return dtype == PBBSS_EVAL_C64 || dtype == PBBSS_EVAL_C128; }
inline bool eval_is_f64(int dtype) { return dtype == PBBSS_EVAL_F64 || dtype == PBBSS_EVAL_C128; }
// can one launch cover B items of N samples (at most kEvalMaxWorkgroups workgroups)?
bool eval_grid_ok(int64_t B, int64_t N);

// doubles of workspace the calls below carve (one partial per item, span and accumulator)
size_t signal_power_work(int64_t rows, int64_t length, int dtype);
size_t si_sdr_work(int64_t B, int Kr, int Ke, int64_t N);

int launch_signal_power(const void* x, int dtype, int64_t rows, int64_t length, int64_t row_stride,
                        double* work, double* out, hipStream_t s);
int launch_si_sdr(const EvalRows& g, double* work, double* out, hipStream_t s);
// work_images / work_noise: signal_power_work doubles of the two arrays
int launch_output_sxr(const void* contributions, const void* noise, int dtype, int64_t B, int Ks,
                      int Kt, int64_t N, int average_sources, double* work_images,
                      double* work_noise, double* out_sxr, int64_t* out_selection, double* out_mean,
                      hipStream_t s);
int launch_input_sxr(const void* images, const void* noise, int dtype, int64_t B, int K, int D,
                     int64_t N, int average_sources, int average_channels, double* work_images,
                     double* work_noise, double* out, hipStream_t s);

}  // namespace pbbss
