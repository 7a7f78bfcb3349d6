"""Speech-to-reverberation modulation energy ratio (reference:
pb_bss/evaluation/module_srmr.py) on the device.  The one metric of `OutputMetrics` that needs
no clean source.

Per call: the voice activity detection and normalisation (`pbbss_srmr_vad`), the gammatone
filterbank (`pbbss_gammatone`), the analytic signal (torch.fft in complex128, the multiplier of
scipy.signal.hilbert, per group of rows that kept the same number of samples -- the one host
read of the call), the eight modulation filters with the frame energies
(`pbbss_srmr_energies`) and the scalar tail (`pbbss_srmr_score`); DESIGN 4.14.

Differences from the reference: float32 rows are widened to float64, not computed in float32; a
list or stacked input is one batched call, not a Python loop; more than 64 cochlear filters
raise NotImplementedError.
"""
import math

import numpy as np

from .. import _lib
from ..transform import gammatone

MODULATION_FREQUENCIES = (4.0, 6.5, 10.7, 17.6, 28.9, 47.5, 78.1, 128.0)
MIN_SAMPLE_RATE = 1000  # below, the frame length int(sample_rate / 1000) * 256 is 0


def modulation_coefficients(sample_rate):
    """(8, 5) float64: b0 b1 b2 a1 a2 of the second-order band-passes (Q = 2) at the eight
    modulation frequencies"""
    coef = np.zeros((len(MODULATION_FREQUENCIES), 5))
    for k, frequency in enumerate(MODULATION_FREQUENCIES):
        w0 = math.tan(2 * math.pi * frequency / (2 * sample_rate))
        b0 = w0 / 2
        norm = 1 + b0 + w0 ** 2
        coef[k] = [b0 / norm, 0, -b0 / norm, (2 * w0 ** 2 - 2) / norm, (1 - b0 + w0 ** 2) / norm]
    return coef


def modulation_cutoffs(sample_rate):
    """(8,) float64: the lower edges of the modulation bands the bandwidth is compared with"""
    cutoffs = []
    for frequency in MODULATION_FREQUENCIES:
        b0 = math.tan(2 * math.pi * frequency / sample_rate / 2) / 2
        cutoffs.append(frequency - (b0 * sample_rate / (2 * math.pi)))
    return np.array(cutoffs)


def vad_rows(x, sample_rate):
    """x: contiguous (rows, N) float32 / float64 device tensor -> (the kept samples of every row,
    normalised, (rows, N) float64 with zeros beyond; the kept lengths, int32 (rows))"""
    t = _lib.torch()
    rows, N = x.shape
    out = t.empty((rows, N), dtype=t.float64, device=x.device)
    lengths = t.empty((rows,), dtype=t.int32, device=x.device)
    _lib.launch('pbbss_srmr_vad', x.device, x, x.dtype == t.float64, rows, N, sample_rate, out,
                lengths, what=f'srmr vad (rows={rows}, N={N}, sample_rate={sample_rate})')
    return out, lengths


def analytic_rows(bands, lengths_host):
    """bands (n, rows, N) float64 -> the analytic signal of every row over its own length,
    complex128 (n, rows, N).  One transform per group of rows of equal length."""
    t = _lib.torch()
    n, rows, N = bands.shape
    groups = {}
    for row, length in enumerate(lengths_host):
        groups.setdefault(int(length), []).append(row)
    out = None
    for length, members in groups.items():
        h = t.zeros((length,), dtype=t.float64, device=bands.device)
        if length % 2 == 0:
            h[0] = h[length // 2] = 1
            h[1:length // 2] = 2
        else:
            h[0] = 1
            h[1:(length + 1) // 2] = 2
        whole = len(members) == rows
        part = bands[:, :, :length] if whole else bands[:, members, :length]
        analytic = t.fft.ifft(t.fft.fft(part.to(t.complex128), dim=-1) * h, dim=-1)
        if whole and length == N:
            return analytic
        if out is None:
            out = t.zeros((n, rows, N), dtype=t.complex128, device=bands.device)
        out[:, members, :length] = analytic
    return out


def _srmr_rows(x, sample_rate, n, low_freq):
    """x: contiguous (rows, N) device tensor -> (rows,) float64 device tensor"""
    t = _lib.torch()
    rows, N = x.shape
    cfs =gammatone.calculate_cfs(low_freq, sample_rate / 2, n)
    # one upload: gammatone stages, modulation filters, ERBs, cutoffs
    host = np.concatenate([
        gammatone.biquad_coefficients(cfs, sample_rate).ravel(),
        modulation_coefficients(sample_rate).ravel(), gammatone.erb(cfs),
        modulation_cutoffs(sample_rate)])
    table = _lib.to_device(host, device=x.device)
    sizes = [n * 20, 40, n, 8]
    gamma_coef, mod_coef, erbs, cutoffs = t.split(table, sizes)
    gamma_coef = gamma_coef.reshape(n, 4, 5)

    y, lengths = vad_rows(x, sample_rate)
    bands = gammatone.filterbank_rows(y, lengths, gamma_coef)
    analytic = analytic_rows(bands, lengths.cpu().tolist()).contiguous()
    means = t.empty((rows, n, 8), dtype=t.float64, device=x.device)
    _lib.launch('pbbss_srmr_energies', x.device, analytic, rows, N, lengths, n, sample_rate,
                mod_coef, means, what=f'srmr energies (rows={rows}, N={N}, n={n})')
    out = t.empty((rows,), dtype=t.float64, device=x.device)
    _lib.launch('pbbss_srmr_score', x.device, means, rows, n, erbs, cutoffs, out,
                what=f'srmr score (rows={rows}, n={n})')
    return out


def _device_srmr(signal, sample_rate, n, low_freq):
    like_torch = _lib.is_torch(signal)
    if not like_torch:
        signal = np.asarray(signal)
    ndim = signal.dim() if like_torch else signal.ndim
    if ndim == 0:
        raise NotImplementedError(ndim)
    for i in range(ndim - 1):
        assert signal.shape[i] < 30, (i, tuple(signal.shape))
    if n > gammatone.MAX_CHANNELS:
        raise NotImplementedError(f'{n} cochlear filters: at most {gammatone.MAX_CHANNELS}')
    if sample_rate != int(sample_rate):
        raise ValueError(f'sample_rate must be a whole number, not {sample_rate}')
    sample_rate = int(sample_rate)
    if sample_rate < MIN_SAMPLE_RATE:
        raise NotImplementedError(f'sample_rate {sample_rate}: the frame length is 0 below 1000')
    home = signal.device if like_torch else None
    x, shape = gammatone.device_rows(signal)
    t = _lib.torch()
    if x.numel() == 0:
        if shape[-1] == 0:
            raise ValueError(f'empty signal: shape {shape}')
        out = t.empty((0,), dtype=t.float64, device=x.device)
    else:
        out = _srmr_rows(x, sample_rate, n, low_freq)
    out = out.reshape(shape[:-1])
    if like_torch:
        return out if out.device == home else out.to(home)
    return _lib.to_host(out)[()]


def srmr(signal, sample_rate: int = 16000, n_cochlear_filters: int = 23, low_freq: int = 125):
    """SRMR of every row of `signal` (samples along the last axis; every leading axis shorter
    than 30, as the reference asserts).  Like the reference, without the active-speech-level
    adjustment of the Matlab SRMRToolbox.

    NumPy (or a list of rows) in gives NumPy out; a device tensor in gives a float64 tensor
    shaped like signal.shape[:-1] on the same device, enqueued on the current stream.  A row
    without a non-zero sample gives nan."""
    return _device_srmr(signal, sample_rate, n_cochlear_filters, low_freq)


def SRMR(signal, sample_rate: int = 16000, n: int = 23, low_freq: int = 125):
    """`srmr` under the name and with the parameter names of the reference's single-row
    function; leading axes are served here as well."""
    return _device_srmr(signal, sample_rate, n, low_freq)
