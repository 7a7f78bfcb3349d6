"""Gammatone filterbank (reference: pb_bss/transform/gammatone.py) on the device.

Every channel is a cascade of four biquads (Slaney's Apple TR #35 design).  The coefficients are
computed here, on the host, in float64; the filtering is one call into csrc/srmr.hip
(`pbbss_gammatone`), where each of the `rows x n` cascades is split along time over the lanes
of a wavefront.  float32 rows are widened at the load, not computed in float32.
"""
import math

import numpy as np

from .. import _lib

MAX_CHANNELS = 64  # csrc/srmr.hpp: kSrmrMaxChannels
EAR_Q = 9.26449    # Glasberg and Moore
MIN_BW = 24.7


def Hz_2_ERBS(f):
    return 21.4 * math.log(0.00437 * f + 1, 10)


def ERBS_2_Hz(f):
    return (10 ** (f / 21.4) - 1) / 0.00437


def calculate_cfs(low_f, high_f, n):
    """`n` centre frequencies in Hz, equally spaced on the ERBS scale from `low_f` up to, but
    not including, `high_f`."""
    low, high = Hz_2_ERBS(low_f), Hz_2_ERBS(high_f)
    step = (high - low) / n
    cfs = np.empty((n,))
    for i in range(n):
        cfs[i] = ERBS_2_Hz(low + i * step)
    return cfs


def erb(cfs):
    """equivalent rectangular bandwidth in Hz at the centre frequencies `cfs`"""
    return np.asarray(cfs) / EAR_Q + MIN_BW


def biquad_coefficients(cfs, sample_rate):
    """(n, 4, 5) float64: b0 b1 b2 a1 a2 of the four cascaded stages of every channel.  All four
    share the pole pair exp(-B T) exp(+-j 2 pi cf T); their zeros differ, and the first stage
    carries the channel's gain."""
    cfs = np.asarray(cfs, dtype=np.float64)
    T = 1 / sample_rate
    B = 1.019 * 2 * math.pi * erb(cfs)
    phase = 2 * cfs * math.pi * T
    decay = np.exp(B * T)
    cos, sin = np.cos(phase), np.sin(phase)
    a1 = -2 * cos / decay
    a2 = np.exp(-2 * B * T)
    roots = [(3 + 2 ** 1.5) ** 0.5, -(3 + 2 ** 1.5) ** 0.5, (3 - 2 ** 1.5) ** 0.5,
             -(3 - 2 ** 1.5) ** 0.5]
    b1 = [-(T * cos / decay + r * (T * sin / decay)) for r in roots]

    rotation = np.exp(2j * phase)
    c1 = -2 * rotation * T
    c2 = 2 * np.exp(-B * T + 1j * phase) * T
    numerator = np.ones_like(c1)
    for r in (roots[3], roots[2], roots[1], roots[0]):
        numerator = numerator * (c1 + c2 * (cos + r * sin))
    denominator = (-2 / np.exp(2 * B * T) - 2 * rotation + 2 * (1 + rotation) / decay) ** 4
    gain = np.abs(numerator / denominator)

    coef = np.zeros((len(cfs), 4, 5))
    for stage in range(4):
        scale = gain if stage == 0 else 1.0
        coef[:, stage, 0] = T / scale
        coef[:, stage, 1] = b1[stage] / scale
        coef[:, stage, 3] = a1
        coef[:, stage, 4] = a2
    return coef


def _check_channels(n):
    if n > MAX_CHANNELS:
        raise NotImplementedError(f'{n} gammatone channels: at most {MAX_CHANNELS}')


def filterbank_rows(x, lengths, coef):
    """x: contiguous (rows, N) float32 / float64 device tensor; lengths: int32 device tensor
    (rows) or None; coef: (n, 4, 5) float64 device tensor -> (n, rows, N) float64, zeros beyond
    a row's length.  Enqueued on the current stream."""
    t = _lib.torch()
    rows, N = x.shape
    n = coef.shape[0]
    out = t.empty((n, rows, N), dtype=t.float64, device=x.device)
    _lib.launch('pbbss_gammatone', x.device, x, x.dtype == t.float64, rows, N, lengths, n, coef,
                out, what=f'gammatone_filterbank(rows={rows}, N={N}, n={n})')
    return out


def device_rows(signal):
    """NumPy array, sequence or tensor -> (contiguous (rows, N) float32 / float64 device tensor,
    shape of the input); a 0-d input comes back as it is"""
    t = _lib.require_gpu()
    if _lib.is_torch(signal):
        x = signal if signal.is_cuda else signal.to(t.device('cuda', t.cuda.current_device()))
    else:
        arr = np.asarray(signal)
        if arr.dtype not in (np.float32, np.float64):
            arr = arr.astype(np.float64)
        x = t.from_numpy(np.ascontiguousarray(arr)).to(t.device('cuda', t.cuda.current_device()))
    if x.dtype not in (t.float32, t.float64):
        if x.dtype.is_complex:
            raise TypeError(f'complex signal ({x.dtype}) where a real one is expected')
        x = x.to(t.float64)
    shape = tuple(x.shape)
    if not shape:  # the callers refuse a signal without a sample axis
        return x, shape
    rows = int(np.prod(shape[:-1], dtype=np.int64))
    return x.reshape(rows, shape[-1]).contiguous(), shape


def gammatone_filterbank(signal, sample_rate=16000, n=23, low_freq=125, high_freq=0):
    """`signal` through `n` gammatone filters whose centre frequencies are equally spaced on the
    ERBS scale from `low_freq` up to (not including) `high_freq`, by default sample_rate / 2.
    The samples run along the last axis; leading axes are independent rows.

    NumPy in gives a list of `n` float64 arrays shaped like `signal`, as the reference returns;
    a device tensor in gives one float64 tensor (n, *signal.shape) on the same device, enqueued
    on the current stream without a host synchronisation.  More than 64 channels:
    NotImplementedError."""
    if high_freq == 0:
        high_freq = sample_rate / 2
    _check_channels(n)
    like_torch = _lib.is_torch(signal)
    home = signal.device if like_torch else None
    x, shape = device_rows(signal)
    if len(shape) == 0:
        raise ValueError('gammatone_filterbank needs a sample axis')
    t = _lib.torch()
    if x.numel() == 0 or n == 0:
        out = t.zeros((n,) + shape, dtype=t.float64, device=x.device)
    else:
        coef = biquad_coefficients(calculate_cfs(low_freq, high_freq, n), sample_rate)
        out = filterbank_rows(x, None, _lib.to_device(coef, device=x.device)).reshape((n,) + shape)
    if like_torch:
        return out if out.device == home else out.to(home)
    return list(_lib.to_host(out))

