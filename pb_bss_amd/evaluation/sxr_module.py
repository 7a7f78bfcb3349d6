"""SNR and invasive SxR of time signals (reference: pb_bss/evaluation/sxr_module.py) on the
device.

`input_sxr` and `output_sxr` are one call into csrc/eval.hip each (`pbbss_input_sxr`,
`pbbss_output_sxr`): the signal powers in one read of the samples, the selection search and the
ratios in a small kernel behind it, no tensor op in between.  `get_snr` takes its two powers
from `pbbss_signal_power` and forms the ratio of the (few) results with one tensor expression.
NumPy in gives NumPy out; a device tensor (float32, float64, complex64 or complex128, widened
in registers) gives float64 tensors on the same device, enqueued on the current stream without
a host synchronisation.  Beyond the reference, `input_sxr` and `output_sxr` take leading batch
axes, and `output_sxr` can return the selection it found.
"""
import collections
import operator

import numpy as np

from .. import _lib
from . import _signals

__all__ = ['get_snr', 'input_sxr', 'output_sxr']


ResultTuple = collections.namedtuple('SXR', ['sdr', 'sir', 'snr'])

_MAX_TARGETS = 8  # output_sxr: 8! = 40 320 selections (csrc/eval.hpp: kSxrMaxTargets)


def _power(x, axis, keepdims):
    """mean of re^2 + im^2 over `axis` (None: all axes) of a device tensor -> float64 tensor"""
    t = _lib.torch()
    nd = x.dim()
    if axis is None:
        reduced = list(range(nd))
    else:
        if not isinstance(axis, (tuple, list)):
            axis = (axis,)
        reduced = []
        for a in axis:
            a = operator.index(a)
            if not -nd <= a < nd:
                raise IndexError(f'axis={a} is out of bounds for an array of dimension {nd}')
            reduced.append(a % nd)
        if len(set(reduced)) != len(reduced):
            raise ValueError(f'axis={tuple(axis)} repeats an axis')
        reduced.sort()
    kept = [a for a in range(nd) if a not in reduced]
    kept_shape = [x.shape[a] for a in kept]
    rows = int(np.prod(kept_shape, dtype=np.int64))
    length = int(np.prod([x.shape[a] for a in reduced], dtype=np.int64))
    if length == 0:
        raise ValueError(f'empty signal: shape {tuple(x.shape)}')
    out = t.empty((rows,), dtype=t.float64, device=x.device)
    if rows:
        xc = x.permute(kept + reduced).contiguous()  # the rows in front; a copy only if needed
        _lib.launch('pbbss_signal_power', x.device, _lib.view_ptr(xc), _signals.dtype_code(xc),
                    rows, length, length, out,
                    what=f'signal_power(shape={tuple(x.shape)}, axis={axis})')
    if keepdims:
        return out.reshape([1 if a in reduced else x.shape[a] for a in range(nd)])
    return out.reshape(kept_shape)


def get_variance_for_zero_mean_signal(X, axis=None, keepdims=False):
    """Mean of re^2 + im^2 over `axis` (sxr_module.py:17-23): the variance of a signal whose mean
    is zero, real or complex, every axis by default.  float64."""
    like_torch, home = _signals.home_of(X)
    x = _signals.device_signal(X, complex_ok=True)
    return _signals.result(_power(x, axis, keepdims), like_torch, home)


def get_snr(X, N, *, axis=None, keepdims=False):
    """10 log10 of the power of `X` over the power of `N` (sxr_module.py:26-48), power being
    the mean of re^2 + im^2 over `axis` -- every axis by default, so arrays of any shape give one
    figure.  `X` and `N` need the same shape only on the axes that are kept.  float64; an axis
    given in `axis` stays with length one under `keepdims`."""
    like_torch, home = _signals.home_of(X, N)
    t = _lib.require_gpu()
    x = _signals.device_signal(X, complex_ok=True)
    n = _signals.device_signal(N, complex_ok=True)
    power_X = _power(x, axis, keepdims)
    power_N = _power(n, axis, keepdims).to(power_X.device)
    return _signals.result(10 * t.log10(power_X / power_N), like_torch, home)


def set_snr(X, N, snr, current_snr=None, *, axis=None, inplace=True):
    """Scale the noise `N` so that `get_snr(X, N, axis=axis)` becomes `snr` dB
    (sxr_module.py:51-79).  Only the noise is touched: `inplace=True` multiplies `N` itself
    (array or tensor) and returns nothing, `inplace=False` leaves it alone and returns `X` with
    a scaled copy.  `current_snr` skips the measurement when the caller knows it; measured, it
    is taken over `axis` with the axes kept, so `snr` may hold one target per kept index."""
    measured = get_snr(X, N, axis=axis, keepdims=True) if current_snr is None else current_snr
    if _lib.is_torch(measured) and isinstance(snr, np.ndarray):
        snr = _lib.torch().as_tensor(snr, device=measured.device)
    gain = 10 ** ((measured - snr) / 20)  # amplitude factor for a power ratio in dB
    if _lib.is_torch(N):
        gain = (gain if _lib.is_torch(gain) else _lib.torch().as_tensor(gain)).to(N.device)
    elif _lib.is_torch(gain):
        gain = _lib.to_host(gain)
    if not inplace:
        return X, N * gain
    N *= gain


def _pair(first, second, first_core, what):
    """the two signal arrays of an sxr call on the device in one dtype, contiguous; the shared
    leading batch shape"""
    like_torch, home = _signals.home_of(first, second)
    a = _signals.device_signal(first, complex_ok=True)
    b = _signals.device_signal(second, complex_ok=True)
    if b.device != a.device:
        b = b.to(a.device)
    a, b = _signals.common_dtype(a, b)
    batch = tuple(a.shape[:-first_core])
    if tuple(b.shape[:-2]) != batch:
        raise ValueError(f'{what}: leading axes {batch} and {tuple(b.shape[:-2])} differ')
    return a.contiguous(), b.contiguous(), batch, like_torch, home


def _returned(values, return_dict):
    """the three results as the `SXR` tuple (return_dict false), or as a dict keyed 'sdr', 'sir',
    'snr' -- behind the prefix when return_dict is a str (sxr_module.py:155-165)"""
    if not return_dict:
        return ResultTuple(*values)
    if return_dict is not True and not isinstance(return_dict, str):
        raise TypeError(return_dict)
    prefix = '' if return_dict is True else return_dict
    return {prefix + field: value for field, value in zip(ResultTuple._fields, values)}


def input_sxr(
        images,
        noise,
        average_sources=True,
        average_channels=True,
        *,
        return_dict=False
):
    """SDR, SIR and SNR in dB of the unmixed signals at the microphones (sxr_module.py:94-165).

    `images` (..., K, D, T) holds each speaker as it arrives at each of the D sensors, `noise`
    (..., D, T) the noise there; both are taken before they are summed into the observation.
    The power of a speaker at a sensor is set against the power of the other speakers (SIR), of
    the noise (SNR) and of both together (SDR).  `average_channels` averages the three powers
    over the sensors before the ratios are formed; `average_sources` averages the dB values over
    the speakers afterwards.  One speaker has no interferer: SIR is inf.

    Returns the `SXR` tuple (sdr, sir, snr); `return_dict=True` a dict with these keys, a str
    the same dict with that str in front of every key.  Each value has the shape
    (..., [K], [D]) without the averaged axes.
    """
    shape = tuple(images.shape)
    noise_shape = tuple(noise.shape)
    assert len(shape) >= 3, (shape, noise_shape)
    K, D, T = shape[-3:]  # Number of speakers, sensors, samples

    assert (D, T) == noise_shape[-2:], ((D, T), shape, noise_shape)
    assert K < 10, shape
    assert D < 30, shape

    x, n, batch, like_torch, home = _pair(images, noise, 3, 'input_sxr')
    t = _lib.torch()
    B = int(np.prod(batch, dtype=np.int64))
    Ko = 1 if average_sources else K
    Do = 1 if average_channels else D
    out = t.empty((B, 3, Ko, Do), dtype=t.float64, device=x.device)
    if B:
        if K == 0 or D == 0 or T == 0:
            raise ValueError(f'empty signal: shape {shape}')
        _lib.launch('pbbss_input_sxr', x.device, x, n, _signals.dtype_code(x), B, K, D, T,
                    bool(average_sources), bool(average_channels), out,
                    what=f'input_sxr(shape={shape})')
    tail = (() if average_sources else (K,)) + (() if average_channels else (D,))
    values = [_signals.result(out[:, m].reshape(batch + tail), like_torch, home) for m in range(3)]
    return _returned(values, return_dict)


def output_sxr(image_contribution, noise_contribution, average_sources=True,
               return_dict=False, *, return_selection=False):
    """SDR, SIR and SNR in dB at the outputs of a separation system, measured invasively
    (sxr_module.py:168-274).

    The caller runs the system once on the mixture, freezes what it estimated (masks, filters)
    and applies that to every clean image and to the noise alone.  `image_contribution`
    (..., K_source, K_target, T) is what source k leaves in output t, `noise_contribution`
    (..., K_target, T) what the noise leaves there.  Each source is assigned an output of its
    own: of all ordered picks of K_source among the K_target outputs, the one whose summed
    power of source k in its output is largest, the first in `itertools.permutations` order
    among equals.  In its output a source is set against the other sources (SIR), the noise
    (SNR) and both (SDR).  1 <= K_source <= K_target <= 8.

    `average_sources` returns the mean of the dB values over the sources, shape (...), instead
    of (..., K_source).  `return_dict=True` returns a dict keyed 'sdr', 'sir', 'snr'; anything
    else, a str prefix included, returns the `SXR` tuple -- that is what the reference's code
    does, whatever its docstring says.  `return_selection=True` returns (result, selection) with
    the (..., K_source) int64 outputs picked, which a caller needs to reorder its estimates.
    """
    shape = tuple(image_contribution.shape)
    noise_shape = tuple(noise_contribution.shape)
    assert len(shape) >= 3, (shape, noise_shape)
    K_source, K_target, samples = shape[-3:]

    assert noise_shape[-2:] == (K_target, samples), (shape, noise_shape)
    assert K_source < 10, (shape, noise_shape)
    assert K_target < 10, (shape, noise_shape)
    # no selection of K_source different targets exists (the reference's selection table is
    # empty and its shape assert fails)
    assert K_source <= K_target, (shape, noise_shape)
    if K_target > _MAX_TARGETS:
        raise NotImplementedError(
            f'{K_target} target speakers: the output_sxr kernel searches the selections of at '
            f'most {_MAX_TARGETS}')

    x, n, batch, like_torch, home = _pair(image_contribution, noise_contribution, 3, 'output_sxr')
    t = _lib.torch()
    B = int(np.prod(batch, dtype=np.int64))
    out = t.empty((B, 3, K_source), dtype=t.float64, device=x.device)
    selection = t.empty((B, K_source), dtype=t.int64, device=x.device)
    mean = t.empty((B, 3), dtype=t.float64, device=x.device) if average_sources else None
    if B:
        if K_source == 0 or samples == 0:
            raise ValueError(f'empty signal: shape {shape}')
        _lib.launch('pbbss_output_sxr', x.device, x, n, _signals.dtype_code(x), B, K_source,
                    K_target, samples, bool(average_sources), out, selection, mean,
                    what=f'output_sxr(shape={shape})')
    if average_sources:
        values = [mean[:, m].reshape(batch) for m in range(3)]
    else:
        values = [out[:, m].reshape(batch + (K_source,)) for m in range(3)]
    values = [_signals.result(v, like_torch, home) for v in values]

    returned = _returned(values, return_dict is True)  # a str prefix counts as false here
    if return_selection:
        return returned, _signals.result(selection.reshape(batch + (K_source,)), like_torch, home)
    return returned
