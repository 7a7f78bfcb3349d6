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

Frame-recursive (online) WPE
----------------------------
``recursive_wpe``, ``OnlineWPE`` and ``online_wpe_step`` keep the names of the package's second
half: one recursive-least-squares update of the filter per frame.  As for the offline half,
neither nara_wpe nor its source is available to this repository: this docstring is the
specification (restated in NumPy by tests/oracle_wpe_online.py), and equality with the package's
output is not checked anywhere.

The stacked past ``ytilde_t`` is exactly the offline one: tap k of sensor d at index ``k D + d``
reads frame ``t - delay - k``; frames before the stream are zeros.  The window therefore starts at
``t - delay`` as offline, which is what makes the recursion equal the batch solution below; the
``delay + 1`` convention that the package's online code is remembered to use could not be checked
here.  State: ``inv_cov`` P (M, M) complex128, Hermitian, initially I; ``filter_taps`` G (M, D)
complex128, initially 0.  Per frame, in this order::

    x_t  = y_t - G^H ytilde_t               (the a-priori error: the output frame)
    n    = P ytilde_t
    den  = alpha lambda_t + Re(ytilde_t^H n)
    k    = n (1 / den)           (k = 0 where den is not > 0: an all-zero stretch)
    P   <- (P - k n^H) (1 / alpha)   only the lower triangle is computed, the diagonal is kept
                                     real, the upper triangle IS the conjugate mirror
    G   <- G + k x_t^H

``lambda_t`` is ``power_estimate[..., t]`` (float64, positive) where the caller gives one, else
the causal power: the mean of |y|^2 over the sensors and over the frames ``t - taps - delay .. t``
of the stream that exist, summed in ascending frame order, so that it does not depend on how the
stream is cut into blocks.  The Hermitian mirror is part of the definition: the antisymmetric
rounding residue of a full-matrix update is divided by alpha every frame and grows like alpha^-t.

Two consequences: with P = I and G = 0 at the start, after T frames ``G = (alpha^T I + R)^-1 C``
with ``R, C = get_correlations(Y, w, taps, delay)`` for the weights
``w_t = alpha^(T - 1 - t) / lambda_t``; and a stream fed in blocks of any lengths gives, bit for
bit, what one call gives.  The state carries the last ``taps + delay`` frames (``history``,
(..., D, taps + delay), newest last) and the number of frames seen.  Served: the offline bounds
and D * (taps + delay) <= 2048.  If ``den``, the output frame, P or G stops being finite the
problem is flagged (``PBBSS_ST_NONFINITE``): its output from that frame on, P and G are NaN; the
other problems of the call are unaffected.  The status words of a call are ``state.status`` of the
returned state and ``OnlineWPE.status`` (a device tensor: reading it is the caller's
synchronisation); ``online_wpe_step`` keeps the package's return values and shows a flagged
problem only through its NaN.
"""
import numpy as np

from .. import _lib, engine

__all__ = ['wpe', 'get_power', 'get_power_inverse', 'get_correlations', 'get_filter_matrix',
           'perform_filter_operation', 'recursive_wpe', 'online_wpe_step', 'OnlineWPE',
           'OnlineWPEState']


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


# ---- frame-recursive WPE ------------------------------------------------------------------------
class OnlineWPEState:
    """The state of a stream of B problems, on the device: ``inv_cov`` (B, M, M), ``filter_taps``
    (B, M, D), ``history`` (B, D, taps + delay) complex128 (the last frames, newest last) and
    ``frames_seen`` (B,) int64; ``status`` (B,) int32: the status words of the call that last
    advanced it (``PBBSS_ST_NONFINITE`` for a flagged problem), None before the first one."""

    def __init__(self, inv_cov, filter_taps, history, frames_seen, status=None):
        self.inv_cov, self.filter_taps = inv_cov, filter_taps
        self.history, self.frames_seen, self.status = history, frames_seen, status

    @classmethod
    def initial(cls, B, D, taps, delay, device=None):
        t = _lib.require_gpu()
        engine.wpe_online_served(D, taps, delay)
        if device is None:
            device = t.device('cuda', t.cuda.current_device())
        M = D * taps
        eye = t.eye(M, dtype=t.complex128, device=device)
        return cls(eye.expand(B, M, M).contiguous(),
                   t.zeros((B, M, D), dtype=t.complex128, device=device),
                   t.zeros((B, D, taps + delay), dtype=t.complex128, device=device),
                   t.zeros((B,), dtype=t.int64, device=device))

    def clone(self):
        return OnlineWPEState(self.inv_cov.clone(), self.filter_taps.clone(),
                              self.history.clone(), self.frames_seen.clone(), self.status)


def _power_rows(power_estimate, B, T, device):
    if power_estimate is None:
        return None
    t = _lib.torch()
    return _lib.to_device(power_estimate, t.float64, device=device).reshape(B, T)


def recursive_wpe(Y, taps=10, delay=3, alpha=0.9999, power_estimate=None, *, layout=None,
                  state=None, return_state=False):
    """Dereverberate ``Y`` frame by frame (module docstring); returns ``X`` with the shape, dtype
    and kind of ``Y``, or ``(X, state)`` with ``return_state=True``.

    ``Y``: (..., D, T), or (..., T, D) with ``layout='f t d'``.  ``power_estimate``: (..., T)
    float64, or None for the causal power.  ``state``: an ``OnlineWPEState`` returned by an
    earlier call, to continue its stream; it is not modified.  One kernel launch; no host
    synchronisation for tensor input.
    """
    y, like_torch = _complex_frames(Y)
    if y.numel() == 0:  # nothing to do: the state stays as it is
        D = y.shape[-2] if layout is None else y.shape[-1]
        B = int(np.prod(y.shape[:-2], dtype=np.int64))
        y3 = None
    else:
        y3 = _problems(y, layout)
        B, D, T = y3.shape
    engine.wpe_online_served(D, taps, delay)
    assert 0.0 < alpha <= 1.0, alpha
    state = (OnlineWPEState.initial(B, D, taps, delay, y.device) if state is None
             else state.clone())
    if y3 is None:
        x = y.clone() if like_torch else _lib.to_host(y)
        return (x, state) if return_state else x
    x3, state.status = engine.wpe_online(
        y3, taps, delay, alpha, _power_rows(power_estimate, B, T, y.device), state.inv_cov,
        state.filter_taps, state.history, state.frames_seen)
    x = _result(x3, tuple(y.shape), like_torch, layout)
    return (x, state) if return_state else x


def online_wpe_step(input_buffer, power_estimate, inv_cov, filter_taps, alpha, taps, delay):
    """One frame in functional form, with the package's argument shapes: ``input_buffer``
    (taps + delay + 1, F, D), newest frame last (tap k reads ``input_buffer[-1 - delay - k]``),
    ``power_estimate`` (F,), ``inv_cov`` (F, M, M), ``filter_taps`` (F, M, D) ->
    ``(pred (F, D), inv_cov, filter_taps)``.  The inputs are not modified."""
    t = _lib.torch()
    buf, like_torch = _complex_frames(input_buffer, 'input_buffer')
    assert buf.ndim == 3 and buf.shape[0] == taps + delay + 1, (tuple(buf.shape), taps, delay)
    F, D = buf.shape[1:]
    dev = buf.device
    P = _lib.to_device(inv_cov, t.complex128, device=dev)
    G = _lib.to_device(filter_taps, t.complex128, device=dev)
    if _lib.is_torch(inv_cov) and P.data_ptr() == inv_cov.data_ptr():
        P = P.clone()
    if _lib.is_torch(filter_taps) and G.data_ptr() == filter_taps.data_ptr():
        G = G.clone()
    history = buf[:-1].permute(1, 2, 0).to(t.complex128).contiguous()
    if history.data_ptr() == buf.data_ptr():
        history = history.clone()
    seen = t.full((F,), taps + delay, dtype=t.int64, device=dev)
    x3, _ = engine.wpe_online(buf[-1].unsqueeze(-1), taps, delay, alpha,
                              _power_rows(power_estimate, F, 1, dev), P, G, history, seen)
    pred = x3.squeeze(-1)
    if not like_torch:
        return _lib.to_host(pred), _lib.to_host(P), _lib.to_host(G)
    return pred, P, G


class OnlineWPE:
    """Frame-recursive WPE over ``frequency_bins`` bins of ``channel`` sensors, the state on the
    device: ``step_frame(frame (F, D)) -> (F, D)`` and ``step_block(block (F, Tb, D)) ->
    (F, Tb, D)``, one kernel launch each, no host synchronisation for tensor input.
    ``power_estimate``: None (the causal power of the stream) or one value per bin, (F,).

    Attributes: ``inv_cov`` (F, M, M), ``filter_taps`` (F, M, D), ``buffer``
    (taps + delay, F, D): the frames behind the stream, newest last, and ``status`` (F,) int32:
    the status words of the last call."""

    def __init__(self, taps=10, delay=3, alpha=0.9999, channel=8, frequency_bins=257,
                 power_estimate=None):
        t = _lib.require_gpu()
        assert 0.0 < alpha <= 1.0, alpha
        self.taps, self.delay, self.alpha = taps, delay, alpha
        self.channel, self.frequency_bins = channel, frequency_bins
        self.state = OnlineWPEState.initial(frequency_bins, channel, taps, delay)
        self.power_estimate = None
        if power_estimate is not None:
            self.power_estimate = _lib.to_device(
                power_estimate, t.float64, device=self.state.inv_cov.device).reshape(frequency_bins)

    inv_cov = property(lambda self: self.state.inv_cov)
    filter_taps = property(lambda self: self.state.filter_taps)
    buffer = property(lambda self: self.state.history.permute(2, 0, 1))
    status = property(lambda self: self.state.status)

    def step_block(self, block):
        """block (F, Tb, D) -> the dereverberated block; advances the state."""
        y, like_torch = _complex_frames(block, 'block')
        assert y.shape[0] == self.frequency_bins and y.shape[2] == self.channel and y.ndim == 3, (
            tuple(y.shape), self.frequency_bins, self.channel)
        if y.shape[1] == 0:
            return y.clone() if like_torch else _lib.to_host(y)
        st = self.state
        power = None
        if self.power_estimate is not None:
            power = self.power_estimate[:, None].expand(-1, y.shape[1]).contiguous()
        x3, st.status = engine.wpe_online(
            y.to(st.inv_cov.device).transpose(1, 2), self.taps, self.delay, self.alpha, power,
            st.inv_cov, st.filter_taps, st.history, st.frames_seen)
        x = x3.transpose(1, 2)
        return x if like_torch else _lib.to_host(x)

    def step_frame(self, frame):
        """frame (F, D) -> the dereverberated frame; advances the state."""
        y, like_torch = _complex_frames(frame, 'frame')
        x = self.step_block(y.unsqueeze(1)).squeeze(1)
        return x if like_torch else _lib.to_host(x)
