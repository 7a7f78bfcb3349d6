"""WPE dereverberation (weighted prediction error; Nakatani et al. 2010, Drude et al. 2018) with
the offline signatures of ``nara_wpe.wpe`` -- the package whose ``stft`` / ``istft`` this
subpackage already mirrors -- on the device.

For one problem ``Y`` (D sensors, T frames) and ``M = D * taps``: the stacked past of frame t is
``(y[t - delay], y[t - delay - 1], ..., y[t - delay - taps + 1])`` with zeros before frame 0.
``X = Y``, then ``iterations`` times::

    p_t   = mean_d |x_td|^2            (averaged over psd_context frames on either side)
    w_t   = 1 / max(p_t, 1e-10 max_t p_t)
    R, P  = sum_t w_t ytilde_t ytilde_t^H,  sum_t w_t ytilde_t y_t^H      (always from Y)
    G     = R^-1 P
    x_t   = y_t - G^H ytilde_t

Every leading axis is an independent problem.  NumPy in gives NumPy out, a device tensor in gives
a device tensor out.  Arithmetic is float64 on the widened values; ``X`` has the dtype of ``Y``
(rounded once for complex64); ``R``, ``P``, ``G`` are complex128.  Results are bit-identical from
call to call and a batch gives bitwise what its problems give one at a time.  Served: 1 <= D <= 16
sensors, D * taps <= 96, any T, any number of problems; beyond that ``NotImplementedError`` names
the bound.

Decisions where the package gives NaN or an exception:

* ``iterations=0`` returns a copy of ``Y``.
* A problem whose frames are all zero returns zeros (its weights are 0, not 1 / 0).
* ``delay=0`` is accepted but degenerate: tap 0 predicts the frame itself and ``X`` collapses
  to 0.
* If the Cholesky factorisation of ``R`` meets a pivot that is not positive or not finite, the
  problem is flagged (``PBBSS_ST_NOT_POSDEF``) and its rows of ``X`` are NaN on the device.  With
  ``check`` on -- the default for NumPy input, which is fetched anyway; ``check=True`` for
  tensors, which costs one host synchronisation -- only the flagged problems are redone step by
  step with ``numpy.linalg.lstsq`` on the host in place of the solve (the package's
  solve-then-lstsq fallback).  Exactly singular input (``R = 0``, e.g. ``T <= delay``) then
  gives ``X = Y``.  Numerically rank-deficient input (``T < M``) is outside the tested domain.
"""
import numpy as np

from .. import _lib, engine

__all__ = ['wpe', 'get_power', 'get_power_inverse', 'get_correlations', 'get_filter_matrix',
           'perform_filter_operation']


def _complex_frames(Y, what='Y'):
    """(device tensor, was it a tensor): complex64 / complex128, at least 2-D."""
    t = _lib.torch()
    like_torch = _lib.is_torch(Y)
    dtype = Y.dtype if like_torch else np.asarray(Y).dtype
    ok = (t.complex64, t.complex128) if like_torch else (np.complex64, np.complex128)
    assert dtype in ok, f'{what} must be complex64 or complex128, got {dtype}'
    y = _lib.to_device(Y) if not like_torch or not Y.is_cuda else Y
    assert y.ndim >= 2, tuple(y.shape)
    return y, like_torch


def _problems(y, layout=None):
    """(..., D, T) -- or (..., T, D) for layout 'f t d' -- -> a (B, D, T) view."""
    if layout is not None and layout.replace(' ', '') != 'ftd':
        raise ValueError(f"layout must be None or 'f t d', got {layout!r}")
    y3 = y.reshape((-1,) + tuple(y.shape[-2:]))
    return y3 if layout is None else y3.transpose(1, 2)


def _result(x3, shape, like_torch, layout=None):
    x = (x3 if layout is None else x3.transpose(1, 2)).reshape(shape)
    return x if like_torch else _lib.to_host(x)


def get_power(signal, psd_context=0):
    """(..., D, T) complex -> (..., T) float64: the mean over the sensors of |signal|^2, averaged
    over the frames of [t - psd_context, t + psd_context] that exist (``inf``: over all frames)."""
    y, like_torch = _complex_frames(signal, 'signal')
    power, _ = engine.wpe_power(_problems(y), psd_context, inverse=False)
    return _result(power, tuple(y.shape[:-2]) + (y.shape[-1],), like_torch)


def get_power_inverse(signal, psd_context=0):
    """(..., D, T) complex -> (..., T) float64: 1 / max(power, 1e-10 * max_t power), the maximum
    per problem.  An all-zero problem gets 0."""
    y, like_torch = _complex_frames(signal, 'signal')
    _, inv = engine.wpe_power(_problems(y), psd_context)
    return _result(inv, tuple(y.shape[:-2]) + (y.shape[-1],), like_torch)


def get_correlations(Y, inverse_power, taps, delay, statistics_mode='full'):
    """Y (..., D, T), inverse_power (..., T) -> (R (..., M, M), P (..., M, D)) complex128 with
    M = D * taps, summed over all frames ('full') or over t >= delay + taps - 1 ('valid')."""
    t = _lib.torch()
    y, like_torch = _complex_frames(Y)
    lead, (D, T) = tuple(y.shape[:-2]), y.shape[-2:]
    inv = _lib.to_device(inverse_power, t.float64, device=y.device).reshape(-1, T)
    R, P = engine.wpe_correlations(_problems(y), inv, taps, delay, statistics_mode)
    M = D * taps
    return _result(R, lead + (M, M), like_torch), _result(P, lead + (M, D), like_torch)


def get_filter_matrix(R, P):
    """G = R^-1 P: (..., M, M), (..., M, D) -> (..., M, D) complex128.  Problems whose R is not
    positive definite are solved by ``numpy.linalg.lstsq`` on the host (NumPy input; a tensor
    keeps NaN there)."""
    t = _lib.torch()
    like_torch = _lib.is_torch(P)
    Rd = _lib.to_device(R, t.complex128)
    Pd = _lib.to_device(P, t.complex128, device=Rd.device)
    M, D = Pd.shape[-2:]
    G, status = engine.wpe_filter_matrix(Rd.reshape(-1, M, M), Pd.reshape(-1, M, D))
    if not like_torch:
        _lstsq_flagged(G, status, Rd.reshape(-1, M, M), Pd.reshape(-1, M, D))
    return _result(G, tuple(Pd.shape), like_torch)


def _lstsq_flagged(G, status, R, P):
    """Overwrite G of the flagged problems with the least-squares solution; -> their indices."""
    flagged = np.flatnonzero(_lib.to_host(status))
    for b in flagged:
        Rb, Pb = _lib.to_host(R[b]), _lib.to_host(P[b])
        if np.isfinite(Rb).all() and np.isfinite(Pb).all():
            Gb = np.linalg.lstsq(Rb, Pb, rcond=None)[0]
            G[b] = _lib.to_device(Gb, G.dtype, device=G.device)
    return flagged


def perform_filter_operation(Y, G, taps, delay):
    """x_t = y_t - G^H ytilde_t: Y (..., D, T), G (..., D * taps, D) -> X like Y."""
    t = _lib.torch()
    y, like_torch = _complex_frames(Y)
    D = y.shape[-2]
    Gd = _lib.to_device(G, t.complex128, device=y.device).reshape(-1, D * taps, D)
    x = engine.wpe_apply_filter(_problems(y), Gd, taps, delay)
    return _result(x, tuple(y.shape), like_torch)


def _stepwise(y3, taps, delay, iterations, psd_context, statistics_mode):
    """The iteration step by step with the host's lstsq wherever the device solve is flagged;
    y3 (B, D, T) complex128."""
    x = y3
    for _ in range(iterations):
        _, inv = engine.wpe_power(x, psd_context)
        R, P = engine.wpe_correlations(y3, inv, taps, delay, statistics_mode)
        G, status = engine.wpe_filter_matrix(R, P)
        _lstsq_flagged(G, status, R, P)
        x = engine.wpe_apply_filter(y3, G, taps, delay)
    return x


def wpe(Y, taps=10, delay=3, iterations=3, psd_context=0, statistics_mode='full', *, layout=None,
        check=None):
    """Dereverberate ``Y``; returns ``X`` with the shape, dtype and kind (NumPy / tensor) of ``Y``.

    ``layout=None``: (..., D, T) as in the package.  ``layout='f t d'``: (..., T, D), what
    ``stft(..., layout='f t d')`` writes and ``CACGMMTrainer.fit`` reads; the kernels read either
    through its strides, nothing is transposed in memory.  ``check``: read the status words and
    redo flagged problems on the host (module docstring); default: only for NumPy input.
    """
    t = _lib.torch()
    if statistics_mode not in engine.WPE_STATISTICS:
        raise ValueError(f"statistics_mode must be 'full' or 'valid', got {statistics_mode!r}")
    y, like_torch = _complex_frames(Y)
    assert iterations >= 0, iterations
    y3 = _problems(y, layout)
    if iterations == 0 or y.numel() == 0:
        return y.clone() if like_torch else _lib.to_host(y)
    x3, status = engine.wpe(y3, taps, delay, iterations, psd_context, statistics_mode)
    if check or (check is None and not like_torch):
        flagged = np.flatnonzero(_lib.to_host(status))
        if flagged.size:
            idx = _lib.to_device(flagged, t.int64, device=y.device)
            redo = _stepwise(y3[idx].to(t.complex128), taps, delay, iterations, psd_context,
                             statistics_mode)
            x3[idx] = redo.to(x3.dtype)
    return _result(x3, tuple(y.shape), like_torch, layout)
