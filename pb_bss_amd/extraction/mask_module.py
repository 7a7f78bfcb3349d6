"""Oracle masks from source images (reference: pb_bss/extraction/mask_module.py) on the device.

Every function takes the complex STFT images as a NumPy array (uploaded, computed, downloaded)
or as a device tensor (device tensor out, on the same device) and runs one call into
csrc/masks.hip: `pbbss_mask_pointwise` for the binary, Wiener-like, ratio, amplitude,
phase-sensitive, complex and biased binary masks, `pbbss_mask_lorenz` and `pbbss_mask_quantile`
for the two masks that need an exact per-row order statistic.  Arithmetic is float64 on the
widened input; the result has the reference's dtype.  Contiguous images are read in place in
any axis order the four collapsed axes of the kernels can express -- (..., K, D, F, T) and the
(..., K, F, T, D) of `stft(layout='f t d')` among them -- anything else takes one copy.

Optional axis parameters are `source_axis` (default 0) and `sensor_axis` (default None; where
a mask defines it, the power is pooled over it).  All other axes are independent.
"""
import ctypes
import operator
from typing import Optional

import numpy as np

from .. import _lib

EPS = 1e-18

__all__ = [
    'voiced_unvoiced_split_characteristic',
    'ideal_binary_mask',
    'wiener_like_mask',
    'ideal_ratio_mask',
    'ideal_amplitude_mask',
    'phase_sensitive_mask',
    'ideal_complex_mask',
    'lorenz_mask',
    'quantile_mask',
    'biased_binary_mask',
]

_MAX_SOURCES = 9
_MAX_SENSORS = 34
_MAX_QUANTILES = 8
_NO_POOLING = ('the images are complex and no rule for pooling them over the sensors is defined '
               'for this mask: call it per sensor, or pool the images yourself')


def voiced_unvoiced_split_characteristic(
        frequency_bins: int,
        split_bin: Optional[int] = None,
        width: Optional[int] = None
):
    """Raised-cosine cross-fade between the voiced (low) and the unvoiced (high) bins.
    Host NumPy, as in the reference (mask_module.py:53-87).

    Returns: tuple of the voiced and the unvoiced frequency weights, each (frequency_bins,).
    """
    if split_bin is None:
        split_bin = frequency_bins // 2
    if width is None:
        width = frequency_bins // 5

    transition = 0.5 * (1 + np.cos(np.pi / (width - 1) * np.arange(0, width)))
    start = int(split_bin - width / 2)

    voiced = np.ones(frequency_bins)
    voiced[start - 1:(start + width - 1)] = transition
    voiced[start - 1 + width:len(voiced)] = 0

    unvoiced = 1 - voiced

    return voiced, unvoiced


# ---- host plumbing ------------------------------------------------------------------------------
def _images(signal):
    """-> (complex64 / complex128 device tensor, untouched strides where possible; like_torch;
    the device to return a tensor result on)"""
    t = _lib.require_gpu()
    like_torch = _lib.is_torch(signal)
    if like_torch:
        home = signal.device
        x = signal if signal.is_cuda else signal.to(t.device('cuda', t.cuda.current_device()))
    else:
        home = None
        x = t.from_numpy(np.ascontiguousarray(signal)).to(
            t.device('cuda', t.cuda.current_device()))
    if x.dtype in (t.float32, t.float64):
        # A real array (magnitudes handed to quantile_mask, say) goes in as its complex embedding:
        # one copy of twice the size.  The kernels have no real-input instantiation.
        x = x.to(t.complex64 if x.dtype == t.float32 else t.complex128)
    if x.dtype not in (t.complex64, t.complex128):
        raise TypeError(f'signal must be float32/64 or complex64/128, not {x.dtype}')
    return x, like_torch, home


def _result(out, like_torch, home):
    if like_torch:
        return out if out.device == home else out.to(home)
    return _lib.to_host(out)


def _axis(axis, ndim, what):
    axis = operator.index(axis)
    if not -ndim <= axis < ndim:
        raise IndexError(f'{what}={axis} is out of bounds for an array of dimension {ndim}')
    return axis % ndim


def _real(t, dtype):
    return t.float32 if dtype == t.complex64 else t.float64


def _collapse(axes, groups):
    """axes: [(size, x_stride, out_stride)] slowest first -> at most `groups` merged axes, padded
    in front with (1, 0, 0); None when they cannot be merged that far."""
    merged = []
    for size, xs, os_ in axes:
        if size == 1:
            continue
        if merged:
            psize, pxs, pos = merged[-1]
            if pxs == xs * size and pos == os_ * size:
                merged[-1] = (psize * size, xs, os_)
                continue
        merged.append((size, xs, os_))
    if len(merged) > groups:
        return None
    return [(1, 0, 0)] * (groups - len(merged)) + merged


def _geom(axes4, **fields):
    g = _lib.MaskGeom()
    for i, (size, xs, os_) in enumerate(axes4):
        g.size[i], g.x_stride[i], g.out_stride[i] = size, xs, os_
    g.sources = g.sensors = 1
    for name, value in fields.items():
        setattr(g, name, value)
    return g


def _without(shape, axis):
    return tuple(s for a, s in enumerate(shape) if a != axis)


def _pointwise(mode, signal, source_axis, sensor_axis, eps=0.0, keepdims=False, table=None,
               out_kind='real'):
    x, like_torch, home = _images(signal)
    t = _lib.torch()
    nd = x.dim()
    k_ax = _axis(source_axis, nd, 'source_axis')
    d_ax = None if sensor_axis is None else _axis(sensor_axis, nd, 'sensor_axis')
    if d_ax == k_ax:
        raise ValueError('source_axis and sensor_axis name the same axis')
    K = x.shape[k_ax]
    D = 1 if d_ax is None else x.shape[d_ax]
    if K > _MAX_SOURCES:
        raise NotImplementedError(f'{K} sources: the mask kernels keep at most {_MAX_SOURCES}')
    if D > _MAX_SENSORS:
        raise NotImplementedError(f'{D} sensors: the mask kernels pool at most {_MAX_SENSORS}')
    dtype = {'real': _real(t, x.dtype), 'complex': x.dtype, 'bool': t.uint8}[out_kind]
    out_shape = _without(x.shape, d_ax)
    if K == 0 or D == 0:
        raise ValueError(f'empty source or sensor axis: shape {tuple(x.shape)}')

    def out_axis(a):
        return a - (1 if d_ax is not None and a > d_ax else 0)

    out = t.empty(out_shape, dtype=dtype, device=x.device)
    rest = [a for a in range(nd) if a not in (k_ax, d_ax)]
    axes4 = _collapse([(x.shape[a], x.stride(a), out.stride(out_axis(a))) for a in rest], 4)
    if axes4 is None:
        # more than four strided groups: sources (and sensors) in front, one copy
        front = [k_ax] + ([] if d_ax is None else [d_ax])
        xc = x.permute(front + rest).contiguous()
        res = _pointwise(mode, xc, 0, None if d_ax is None else 1, eps, False, table, out_kind)
        out = res.movedim(0, out_axis(k_ax)).contiguous()
    elif out.numel():
        g = _geom(axes4, sources=K, sensors=D, x_source_stride=x.stride(k_ax),
                  x_sensor_stride=0 if d_ax is None else x.stride(d_ax),
                  out_source_stride=out.stride(out_axis(k_ax)))
        _lib.launch('pbbss_mask_pointwise', x.device, _lib.view_ptr(x), x.dtype == t.complex128,
                    mode, g, eps, table, 0 if table is None else table.shape[-1], out,
                    what=f'mask_pointwise(mode={mode}, shape={tuple(x.shape)})')
    if out_kind == 'bool':
        out = out.view(t.bool)
    if d_ax is not None and keepdims:
        out = out.unsqueeze(d_ax)
    return _result(out, like_torch, home)


def _threshold(signal, sensor_axis, axis, keepdims, launch, targets=None, may_fail=True):
    """Rows = all axes but `axis` (and the pooled sensor axis); launch(x, geom, out, status).
    The status words are read back (one blocking read) only where a row can fail: the quantile
    kernels never set one."""
    x, like_torch, home = _images(signal)
    t = _lib.torch()
    nd = x.dim()
    d_ax = None if sensor_axis is None else _axis(sensor_axis, nd, 'sensor_axis')
    if not isinstance(axis, (tuple, list)):
        axis = (axis,)
    cols = sorted(_axis(a, nd, 'axis') for a in axis)
    if len(set(cols)) != len(cols) or d_ax in cols or not cols:
        raise ValueError(f'axis={tuple(axis)} repeats an axis or names the sensor axis')
    D = 1 if d_ax is None else x.shape[d_ax]
    if D > _MAX_SENSORS:
        raise NotImplementedError(f'{D} sensors: the mask kernels pool at most {_MAX_SENSORS}')
    rows = [a for a in range(nd) if a not in cols and a != d_ax]
    lead = () if targets is None else (targets,)
    out_shape = _without(x.shape, d_ax)
    if x.numel() == 0:
        raise ValueError(f'empty signal: shape {tuple(x.shape)}')
    out = t.empty(lead + out_shape, dtype=_real(t, x.dtype), device=x.device)
    off = len(lead)

    def out_stride(a):
        return out.stride(off + a - (1 if d_ax is not None and a > d_ax else 0))

    def groups(ax):
        return _collapse([(x.shape[a], x.stride(a), out_stride(a)) for a in ax], 2)

    row2, col2 = groups(rows), groups(cols)
    if row2 is None or col2 is None:
        # one copy with the rows in front and the selection axes last
        perm = rows + ([] if d_ax is None else [d_ax]) + cols
        xc = x.permute(perm).contiguous()
        res = _threshold(xc, None if d_ax is None else len(rows),
                         tuple(range(-len(cols), 0)), False, launch, targets, may_fail)
        back = [0] * (len(rows) + len(cols))
        for i, a in enumerate(rows + cols):
            back[a - (1 if d_ax is not None and a > d_ax else 0)] = i
        out = res.permute(list(range(off)) + [off + b for b in back]).contiguous()
    else:
        g = _geom(row2 + col2, sensors=D, x_sensor_stride=0 if d_ax is None else x.stride(d_ax),
                  out_target_stride=out.stride(0) if targets else 0)
        n_rows = row2[0][0] * row2[1][0]
        status = t.zeros((n_rows,), dtype=t.int32, device=x.device)
        launch(x, g, out, status)
        if may_fail and int(status.max().item()) & _lib.MASK_ST_NO_THRESHOLD:
            bad = int((status != 0).sum().item())
            raise ValueError(
                f'lorenz_mask: {bad} of {n_rows} rows have no element below the Lorenz fraction '
                '(an all-zero row, or one element carries the fraction)')
    if d_ax is not None and keepdims:
        out = out.unsqueeze(off + d_ax)
    return _result(out, like_torch, home)


# ---- the masks ----------------------------------------------------------------------------------
def ideal_binary_mask(
        signal: np.ndarray,
        source_axis: int = 0,
        sensor_axis: Optional[int] = None,
        keepdims: bool = False
) -> np.ndarray:
    """One where the source has the largest (sensor-pooled) power, zero elsewhere; among equal
    powers the first source wins, as with np.argmax (mask_module.py:90-136).  The masks sum to
    one over the sources.  Result: real dtype of the images."""
    return _pointwise(_lib.MASK_IBM, signal, source_axis, sensor_axis, keepdims=keepdims)


def wiener_like_mask(
        signal: np.ndarray,
        source_axis: int = 0,
        sensor_axis: Optional[int] = None,
        eps: float = EPS,
        keepdims: bool = False
) -> np.ndarray:
    """Source power over the power of all sources (+ eps), each pooled over `sensor_axis`
    (mask_module.py:139-179)."""
    return _pointwise(_lib.MASK_WIENER, signal, source_axis, sensor_axis, eps, keepdims)


def ideal_ratio_mask(
        signal: np.ndarray,
        source_axis: int = 0,
        sensor_axis: Optional[int] = None,
        eps: float = EPS,
) -> np.ndarray:
    """Source magnitude over the sum of the source magnitudes (+ eps)
    (mask_module.py:182-232)."""
    assert sensor_axis is None, _NO_POOLING
    return _pointwise(_lib.MASK_IRM, signal, source_axis, None, eps)


def ideal_amplitude_mask(
        signal: np.ndarray,
        source_axis: int = 0,
        sensor_axis: Optional[int] = None,
        eps: float = EPS,
) -> np.ndarray:
    """Source magnitude over the magnitude of the complex sum of the sources (+ eps); not
    bounded by one (mask_module.py:235-287)."""
    assert sensor_axis is None, _NO_POOLING
    return _pointwise(_lib.MASK_IAM, signal, source_axis, None, eps)


def phase_sensitive_mask(
        signal: np.ndarray,
        source_axis: int = 0,
        sensor_axis: Optional[int] = None,
        eps: float = EPS,
) -> np.ndarray:
    """|s| / (|o| + eps) cos(angle s - angle o) with o the sum of the sources
    (mask_module.py:290-322), evaluated as Re(s conj(o)) / (|o| (|o| + eps))."""
    assert sensor_axis is None, _NO_POOLING
    return _pointwise(_lib.MASK_PSM, signal, source_axis, None, eps)


def ideal_complex_mask(
        signal: np.ndarray,
        source_axis: int = 0,
        sensor_axis: Optional[int] = None,
) -> np.ndarray:
    """s / o with o the sum of the sources; complex.  A point that is silent in every source is
    0 / 0 = NaN, as in the reference (mask_module.py:325-347)."""
    assert sensor_axis is None, _NO_POOLING
    return _pointwise(_lib.MASK_ICM, signal, source_axis, None, out_kind='complex')


def lorenz_mask(
        signal: np.ndarray,
        *,
        sensor_axis=None,
        axis=(-2, -1),
        lorenz_fraction: float = 0.98,
        weight: float = 0.999,
        keepdims: bool = False,
) -> np.ndarray:
    """Softened mask of the strongest points of each row by the Lorenz-curve criterion
    (mask_module.py:350-417).

    The (sensor-pooled) powers of a row -- all values along `axis` -- are sorted descending; the
    threshold is the power at the last position whose cumulative share of the row's power is
    below `lorenz_fraction`, and the mask is 0.5 + weight / 2 where the power is strictly above
    it, 0.5 - weight / 2 elsewhere.  A row in which no position qualifies (all zero, or one point
    carries the fraction) raises ValueError, as the reference does; finding that out costs one
    read of the per-row status words.
    """
    high, low = 0.5 + weight * (1.0 - 0.5), 0.5 + weight * (0.0 - 0.5)

    def launch(x, g, out, status):
        t = _lib.torch()
        _lib.launch('pbbss_mask_lorenz', x.device, _lib.view_ptr(x), x.dtype == t.complex128, g,
                    lorenz_fraction, high, low, out, out.dtype == t.float64, status,
                    what=f'mask_lorenz(shape={tuple(x.shape)})')

    return _threshold(signal, sensor_axis, axis, keepdims, launch)


def _percentile_index(quantile, n):
    """(lower rank, gamma, negative) of np.percentile(row of n, q) with the reference's q."""
    negative = not quantile >= 0
    q = abs(quantile) * 100 if negative else (1 - quantile) * 100
    if not 0 <= q <= 100:
        raise ValueError(f'quantile={quantile} gives the percentile {q}, outside [0, 100]')
    virtual = (n - 1) * np.true_divide(q, 100)  # NumPy's 'linear' method
    lower = int(np.floor(virtual))
    if lower >= n - 1:
        return n - 1, 0.0, negative
    return lower, float(virtual - lower), negative


def quantile_mask(
        signal: np.ndarray,
        quantile=(0.1, -0.9),
        *,
        sensor_axis=None,
        axis=-2,
        weight: float = 0.999,
) -> np.ndarray:
    """Softened mask of the points of each row above (quantile >= 0: the top `quantile` share)
    or below (quantile < 0: the bottom `|quantile|` share) the row's percentile of |signal|
    (mask_module.py:420-493).  The threshold is NumPy's linearly interpolated percentile; the
    comparison is strict.

    A tuple or list of quantiles gives (len(quantile), *signal.shape), from one selection sweep
    per eight quantiles.  When `axis` names every axis the whole array is one row (the
    reference fails there under NumPy 2: its row count is a float).  A real `signal` is copied
    once into a complex tensor of twice its size before the kernel reads it; complex images are
    read in place.  Nothing but the result is read back from the device.
    """
    assert sensor_axis is None, _NO_POOLING
    t = _lib.torch()
    if isinstance(quantile, (tuple, list)):
        if any(isinstance(q, (tuple, list)) for q in quantile) or len(quantile) == 0:
            parts = [quantile_mask(signal, q, sensor_axis=sensor_axis, axis=axis, weight=weight)
                     for q in quantile]
            if parts and _lib.is_torch(parts[0]):
                return t.stack(parts)
            return np.array(parts)
        if len(quantile) > _MAX_QUANTILES:
            parts = [quantile_mask(signal, list(quantile[i:i + _MAX_QUANTILES]),
                                   sensor_axis=sensor_axis, axis=axis, weight=weight)
                     for i in range(0, len(quantile), _MAX_QUANTILES)]
            return t.cat(parts) if _lib.is_torch(parts[0]) else np.concatenate(parts)
        quantiles, targets = list(quantile), len(quantile)
    else:
        quantiles, targets = [quantile], None
    high, low = 0.5 + weight * (1.0 - 0.5), 0.5 + weight * (0.0 - 0.5)

    def launch(x, g, out, status):
        n = g.size[2] * g.size[3]
        spec = [_percentile_index(q, n) for q in quantiles]
        Q = len(spec)
        rank = (ctypes.c_int64 * Q)(*[s[0] for s in spec])
        gamma = (ctypes.c_double * Q)(*[s[1] for s in spec])
        negative = (ctypes.c_int * Q)(*[int(s[2]) for s in spec])
        _lib.launch('pbbss_mask_quantile', x.device, _lib.view_ptr(x), x.dtype == t.complex128, g,
                    Q, rank, gamma, negative, high, low, out, out.dtype == t.float64, status,
                    what=f'mask_quantile(shape={tuple(x.shape)}, quantile={quantiles})')

    return _threshold(signal, None, axis, False, launch, targets, may_fail=False)


def biased_binary_mask(
        signal: np.ndarray,
        component_axis: int = 0,
        sensor_axis: Optional[int] = None,
        frequency_axis: int = -1,
        threshold_unvoiced_speech: int = 5,
        threshold_voiced_speech: int = 0,
        threshold_unvoiced_noise: int = -10,
        threshold_voiced_noise: int = -10,
        low_cut: int = 5,
        high_cut: int = 500,
) -> np.ndarray:
    """Speech and noise masks (bool) of one speaker (component 0) in noise (component 1) with
    frequency-dependent SNR thresholds in dB (mask_module.py:496-550).

    As in the reference, the thresholds -- a cross-fade over the bins of `frequency_axis` --
    and the cuts apply along the LAST axis, so `frequency_axis` has to have the length of the
    last axis; speech is off and noise on below `low_cut - 1` and from `high_cut` up to the
    length of axis 1 of the masks (the reference writes `len(speech_mask[0])` there; for 2-D
    images that is the number of bins).
    """
    if sensor_axis is not None:
        raise NotImplementedError('biased_binary_mask has no rule for pooling over the sensors')
    shape = tuple(signal.shape)
    nd = len(shape)
    k_ax = _axis(component_axis, nd, 'component_axis')
    assert shape[k_ax] == 2, f'one speaker and noise: 2 components, not {shape[k_ax]}'
    if nd < 2 or k_ax == nd - 1:
        raise NotImplementedError('biased_binary_mask: the last axis must hold the bins')
    bins = shape[_axis(frequency_axis, nd, 'frequency_axis')]
    last = shape[-1]
    if bins != last:
        raise ValueError(f'the thresholds span {bins} bins but apply along the last axis of '
                         f'length {last}')
    voiced, unvoiced = voiced_unvoiced_split_characteristic(bins)
    threshold_speech = threshold_voiced_speech * voiced + threshold_unvoiced_speech * unvoiced
    threshold_noise = threshold_unvoiced_noise * voiced + threshold_voiced_noise * unvoiced
    cut = np.zeros(last)
    cut[0:low_cut - 1] = 1
    mask_shape = list(shape)
    mask_shape[k_ax] = 1
    cut[high_cut:mask_shape[1]] = 1
    table = np.stack([10 ** (threshold_speech / 10), 10 ** (threshold_noise / 10), cut])
    t = _lib.require_gpu()
    device = signal.device if _lib.is_torch(signal) and signal.is_cuda else None
    table = _lib.to_device(table, t.float64, device)
    return _pointwise(_lib.MASK_BIASED, signal, k_ax, None, table=table, out_kind='bool')
