"""Short-time objective intelligibility (reference: pb_bss/evaluation/module_stoi.py, a Python loop
around the `pystoi` package) on the device, float64, without the package (csrc/stoi.hip,
DESIGN 4.16).

Per call: the polyphase resampler to 10 kHz where the sample rate differs (`pbbss_resample_poly`,
once per row that was handed in, not per pair; the window computed here and uploaded) and one
`pbbss_stoi` over all pairs: frame energies, removal of the silent frames, the 512-point
transform, 15 third-octave bands and the segment correlations.  Nothing is read back to the host.

Differences from the reference: float32 rows are widened to float64; all leading axes are one
batched call; a pair with fewer than 30 frames gives pystoi's 1e-5 without its warning, also
where the package raises for a row too short for one frame; `extended=True` is not offered (the
reference's wrapper cannot pass it either).
"""
import functools
import math

import numpy as np

from .. import _lib
from . import _signals

FS = 10000
MAX_LENGTH = 1 << 24  # samples of a row, before and after the resampler (csrc/stoi.hpp)


@functools.lru_cache(maxsize=8)
def resample_window(up, down):
    """the (2 L + 1) taps of Octave's `resample` for the ratio up / down, as pystoi builds them:
    a sinc at fc = 1 / (2 max(up, down)) under a Kaiser window for 60 dB rejection and a roll-off
    of fc / 10, normalised to unit sum"""
    fc = 1.0 / (2 * max(up, down))
    rejection = 60.0
    half = int(math.ceil((rejection - 8.0) / (28.714 * fc / 10)))
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (rejection - 8.7)) * (2 * up * fc * np.sinc(2 * fc * t))
    h = h / np.sum(h)
    h.setflags(write=False)
    return h


def device_window(up, down, device):
    """resample_window(up, down) on the device (a copy: the cached array is read-only)"""
    return _lib.to_device(resample_window(up, down).copy(), device=device)


def resample_rows(x, up, down, window=None):
    """x: contiguous (rows, N) float32 / float64 device tensor -> (rows, ceil(N up / down))
    float64, scipy.signal.resample_poly(x, up, down, window=resample_window(up, down));
    window: device_window(up, down, x.device) where the caller has uploaded it already"""
    t = _lib.torch()
    rows, N = x.shape
    M = -(-N * up // down)
    if max(N, M) > MAX_LENGTH:
        raise NotImplementedError(f'rows of {N} samples ({M} resampled): at most {MAX_LENGTH}')
    if window is None:
        window = device_window(up, down, x.device)
    out = t.empty((rows, M), dtype=t.float64, device=x.device)
    _lib.launch('pbbss_resample_poly', x.device, x, x.dtype == t.float64, rows, N, up, down,
                window, window.numel(), out,
                what=f'resample_poly(rows={rows}, N={N}, up={up}, down={down})')
    return out


def _rows_at_10k(x, N, ratio, window):
    """x (..., N or 1) float32 / float64 -> float64 (..., N10) with a unit stride along the
    samples; the leading axes keep the sizes x came with.  ratio: (up, down), window: its taps
    on the device; both None at 10 kHz"""
    t = _lib.torch()
    if x.shape[-1] != N:  # a broadcast sample axis is written out
        x = x.expand(x.shape[:-1] + (N,))
    if ratio is None:
        x = x.to(t.float64)
        return x if N == 1 or x.stride(-1) == 1 else x.contiguous()
    flat = x.reshape(-1, N).contiguous()
    out = resample_rows(flat, *ratio, window)
    return out.reshape(x.shape[:-1] + (out.shape[-1],))


def stoi_rows(x, y, outer, inner, strides, return_frames=False):
    """`outer * inner` pairs of float64 rows at 10 kHz, pair (o, i) at element offsets
    o strides[0] + i strides[1] of x and o strides[2] + i strides[3] of y -> (outer, inner)
    float64 (and, asked for, int32 (outer, inner, 2): the frames before and after the removal)"""
    t = _lib.torch()
    N10 = x.shape[-1]
    assert x.dtype == t.float64 and y.dtype == t.float64 and y.shape[-1] == N10
    if N10 > MAX_LENGTH:
        raise NotImplementedError(f'rows of {N10} samples: at most {MAX_LENGTH}')
    out = t.empty((outer, inner), dtype=t.float64, device=x.device)
    frames = t.empty((outer, inner, 2), dtype=t.int32, device=x.device) if return_frames else None
    _lib.launch('pbbss_stoi', x.device, _lib.view_ptr(x), _lib.view_ptr(y), outer, inner, N10,
                *strides, out, frames, what=f'stoi(outer={outer}, inner={inner}, N10={N10})')
    return (out, frames) if return_frames else out


def stoi(reference, estimation, sample_rate):
    """STOI of `estimation` (processed) against `reference` (clean), samples along the last axis.

    The two arguments broadcast against each other like np.broadcast_arrays, every leading axis
    in one call: `reference (K, 1, N)` against `estimation (1, D, N)` gives the (K, D) score
    matrix, and rows shared along an axis are read in place (stride 0).  float64, of the shape
    the arguments broadcast to without the sample axis.  NumPy in gives NumPy out (a 0-d result
    as a scalar); a device tensor in gives a tensor on the same device, enqueued on the current
    stream without a host synchronisation.  A pair with fewer than 30 frames at 10 kHz
    (about 4 000 samples after the silent frames are gone) gives 1e-5.
    """
    like_torch, home = _signals.home_of(reference, estimation)
    if sample_rate != int(sample_rate) or int(sample_rate) < 1:
        raise ValueError(f'sample_rate must be a whole number >= 1, not {sample_rate}')
    sample_rate = int(sample_rate)
    t = _lib.require_gpu()
    ref = _signals.device_signal(reference, complex_ok=False)
    est = _signals.device_signal(estimation, complex_ok=False)
    if est.device != ref.device:
        est = est.to(ref.device)
    if ref.dim() == 0 or est.dim() == 0:
        raise ValueError('stoi needs a sample axis')
    shape = tuple(t.broadcast_shapes(ref.shape, est.shape))
    N, lead = shape[-1], shape[:-1]
    if N == 0:
        raise ValueError(f'empty signal: shape {shape}')
    if int(np.prod(lead, dtype=np.int64)) == 0:
        return _signals.result(t.empty(lead, dtype=t.float64, device=ref.device), like_torch, home)

    ratio = window = None
    if sample_rate != FS:  # one upload of the taps per call
        g = math.gcd(FS, sample_rate)
        ratio = (FS // g, sample_rate // g)
        window = device_window(*ratio, ref.device)
    x, y = _rows_at_10k(ref, N, ratio, window), _rows_at_10k(est, N, ratio, window)
    full = lead + (x.shape[-1],)
    xb, yb = x.expand(full), y.expand(full)
    merged = _signals.collapse([(lead[a], xb.stride(a), yb.stride(a)) for a in range(len(lead))])
    if len(merged) > 2:  # more than two independent axes: the pairs written out
        xb, yb = xb.contiguous(), yb.contiguous()
        merged = [(int(np.prod(lead, dtype=np.int64)), full[-1], full[-1])]
    merged = [(1, 0, 0)] * (2 - len(merged)) + merged
    (outer, xo, yo), (inner, xi, yi) = merged
    out = stoi_rows(xb, yb, outer, inner, (xo, xi, yo, yi))
    return _signals.result(out.reshape(lead), like_torch, home)
