/* pbbss_stream.h -- the streaming section of the C ABI of libpbbss_hip.so: entry points whose
 * state lives in tensors of the caller.
 *
 * The functions declared here take a handle of pbbss.h, but only as the name of a device and of
 * its launch limits: they carve nothing from the handle's slabs, control words or team buffer, and
 * leave nothing in it.  Everything a stream carries from call to call (sample history, overlap
 * tail) is device memory that the caller owns and passes in; the counters of a stream are host
 * integers of the caller.  A call may therefore stand anywhere between the calls of pbbss.h on the
 * same handle, and any number of streams may share one handle, as long as the calls on one
 * handle are enqueued on one stream at a time (the rule of pbbss.h).
 *
 * Error codes, the handle and the stream argument are those of pbbss.h, which this header
 * includes; PBBSS_VERSION is not moved by this section.  All pointers are device pointers.
 */
#ifndef PBBSS_STREAM_H_
#define PBBSS_STREAM_H_

#include "pbbss.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One call of a streaming STFT: the block x (C, n) of float32 / float64 samples follows the
 * samples_seen samples the stream has taken so far; the call writes the m frames that the block
 * completes, bit for bit the frames frames_seen .. frames_seen + m - 1 of pbbss_stft on the whole
 * signal (same size, shift, window_length, window, fading), as out (C, m, F) [out_layout 0] or
 * (F, m, C) [out_layout 1], F = size / 2 + 1, complex128 or complex64.
 *
 * hist_in (C, H) float64, H = max(1, window_length - 1): the last H samples in front of the block,
 * newest last, zeros in front of the stream (all zeros before the first call).  hist_out (C, H):
 * ANOTHER buffer, which receives the same for the next call; the caller swaps the two.  The
 * caller then adds n to samples_seen and m to frames_seen.
 *
 * flush = 0: m must be the number of frames the block completes: frame t is complete when
 *   t * shift + window_length <= fade + samples_seen + n, fade = fading ? window_length - shift : 0.
 * flush = 1: n must be 0; the stream ends behind samples_seen and the call writes m more frames,
 *   the samples behind the end read as zeros (the closing fade and the padded last frame: m =
 *   pbbss_stft_num_frames(samples_seen, ...) - frames_seen), and hist_out is zeroed: the
 *   initial state.
 * n = 0 and m = 0 without flush does nothing.  x may be NULL where n = 0, out where m = 0.
 *
 * One launch, no device memory of the handle, no host synchronisation.
 * PBBSS_ERR_INVALID_ARG: NULL pointer, n < 0, counters that do not fit together.
 * PBBSS_ERR_UNSUPPORTED: size not a power of two in [4, 8192], window_length > size, C > 65535. */
PBBSS_API int pbbss_stft_stream(pbbss_handle_t h, const void* x, int x_is_f64, int64_t C, int64_t n,
                                const double* hist_in, double* hist_out, int64_t samples_seen,
                                int64_t frames_seen, int m, int flush, int size, int shift,
                                int window_length, const double* window, int fading, int out_layout,
                                int out_is_c128, void* out, void* stream);

/* One call of a streaming inverse STFT: m frames of `rows` independent rows, complex64 /
 * complex128, element (row, t, k) at X + row * stride_r + t * stride_t + k * stride_f (strides in
 * complex elements, so (rows, m, F) and (rows, F, m) are both read in place).  Each frame
 * completes one hop of `shift` samples; the sums are those of pbbss_istft on the concatenated
 * frames, bit for bit.
 *
 * tail (rows, window_length - shift) float64: the overlap behind the last complete hop, zeros
 * before the first call; read and rewritten (may be NULL where window_length == shift).
 * skip: samples of this call that precede the output, 0 <= skip <= window_length - shift (the
 * fade-in that pbbss_istft drops with fading: max(0, window_length - shift - frames_seen *
 * shift)).  out (rows, n_out) float64 with n_out = max(0, m * shift - skip); may be NULL where
 * n_out = 0.  The closing tail of a stream without fading is the tail buffer itself.
 *
 * One launch, no scratch, no device memory of the handle, no host synchronisation.
 * PBBSS_ERR_INVALID_ARG: NULL pointer, m < 1, window_length no multiple of shift, n_out wrong.
 * PBBSS_ERR_UNSUPPORTED: size not a power of two in [4, 8192], window_length > size,
 * rows > 65535. */
PBBSS_API int pbbss_istft_stream(pbbss_handle_t h, const void* X, int x_is_c128, int64_t rows, int m,
                                 int64_t stride_r, int64_t stride_t, int64_t stride_f, int size,
                                 int shift, int window_length, const double* synthesis_window,
                                 double* tail, int skip, double* out, int64_t n_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PBBSS_STREAM_H_ */
