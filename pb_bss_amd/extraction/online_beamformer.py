"""Frame-recursive (online) mask-driven MVDR beamformer on the device: what produces the
time-dependent vectors that ``apply_online_beamforming_vector`` applies.

No package implements this under this name: the reference only applies such vectors ("emulates an
online system") and never estimates them.  This docstring is the specification (restated in NumPy
by tests/oracle_online_beamformer.py); it is the classic online mask-based MVDR: exponentially
forgotten target and noise statistics, the noise inverse kept by a rank-one (Sherman-Morrison)
update, the Souden vector and its output per frame.

For one problem (one bin) with D sensors and frames ``y_t``: target mask ``s_t >= 0`` and noise
mask ``v_t >= 0`` (float64 after widening), forgetting factor ``0 < alpha <= 1``, reference
channel ``r``, ``p0 = initial_noise_power > 0``.  State: ``target_psd`` Phi (D, D) complex128,
Hermitian, initially 0; ``noise_inv`` Psi (D, D) complex128, Hermitian, initially ``I / p0``.
Per frame, in this order::

    Phi <- alpha Phi + s_t y_t y_t^H          the lower triangle is computed, the diagonal kept
                                              real, the upper triangle IS the conjugate mirror
    n    = Psi y_t
    den  = alpha + v_t Re(y_t^H n)
    Psi <- (Psi - (v_t / den) n n^H) / alpha  same triangle / mirror / real-diagonal rule;
                                              the product is ((v_t / den) n) n^H
    u    = Phi[:, r]
    lam  = sum_ij Re(Psi_ij conj(Phi_ij))     (= Re tr(Psi Phi))
    w_t  = (Psi u) / max(lam, tiny)           tiny = the smallest positive normal float64, the
                                              eps of get_mvdr_vector_souden
    x_t  = w_t^H y_t

The frame's own statistics are in ``w_t`` (a-posteriori).  While Phi is still 0, ``w_t = 0`` and
``x_t = 0``.  Arithmetic is float64 on the widened values; ``x`` has the dtype of ``Y`` (rounded
once for complex64); ``w``, Phi and Psi are complex128.

Two consequences.  After T frames from the initial state ``Phi = sum_t alpha^(T-1-t) s_t y_t
y_t^H``, ``Psi^-1 = alpha^T p0 I + sum_t alpha^(T-1-t) v_t y_t y_t^H`` and ``w_{T-1}`` is
``get_mvdr_vector_souden(Phi, Psi^-1, ref_channel=r)``.  And a stream cut into blocks of any
lengths gives what one call gives, bit for bit, for ``x``, ``w``, Phi and Psi; a batch gives
bitwise what its problems give alone; results are bit-identical from call to call.

A problem is flagged (``PBBSS_ST_NONFINITE`` in ``state.status`` / ``OnlineMVDR.status``) if
``den`` is not > 0, or if ``den``, ``lam`` or ``x_t`` is not finite: its ``x`` and ``w`` from that
frame on are NaN, and so are its Phi and Psi; the other problems of the call are unaffected.
Known limit: with ``alpha < 1`` and no noise-mask mass Psi grows like ``alpha^-t``, as the
mathematics says, and ends in this flag.

Served: 1 <= D <= 16 sensors, any T, any number of problems; beyond that ``NotImplementedError``
names ``ONLINE_BF_MAX_D = 16``.
"""
import numpy as np

from .. import _lib, engine
from ..transform.wpe import _complex_frames, _problems

__all__ = ['recursive_mvdr_souden', 'OnlineMVDR', 'OnlineBeamformerState']


class OnlineBeamformerState:
    """The state of a stream of B problems, on the device: ``target_psd`` and ``noise_inv``
    (B, D, D) complex128, ``frames_seen`` (B,) int64; ``status`` (B,) int32: the status words of
    the call that last advanced it (``PBBSS_ST_NONFINITE`` for a flagged problem), None before the
    first one."""

    def __init__(self, target_psd, noise_inv, frames_seen, status=None):
        self.target_psd, self.noise_inv = target_psd, noise_inv
        self.frames_seen, self.status = frames_seen, status

    @classmethod
    def initial(cls, B, D, initial_noise_power=1.0, device=None):
        t = _lib.require_gpu()
        engine.online_bf_served(D)
        assert D >= 1 and initial_noise_power > 0.0, (D, initial_noise_power)
        if device is None:
            device = t.device('cuda', t.cuda.current_device())
        eye = t.eye(D, dtype=t.complex128, device=device) / initial_noise_power
        return cls(t.zeros((B, D, D), dtype=t.complex128, device=device),
                   eye.expand(B, D, D).contiguous(),
                   t.zeros((B,), dtype=t.int64, device=device))

    def clone(self):
        return OnlineBeamformerState(self.target_psd.clone(), self.noise_inv.clone(),
                                     self.frames_seen.clone(), self.status)


def _mask_rows(target_mask, noise_mask, B, T, device):
    """Both masks as (B, T) device tensors of one dtype: float32 if both are, else float64."""
    t = _lib.torch()

    def kind(m):
        dtype = m.dtype if _lib.is_torch(m) else np.asarray(m).dtype
        ok = (t.float32, t.float64) if _lib.is_torch(m) else (np.float32, np.float64)
        assert dtype in ok, f'masks must be float32 or float64, got {dtype}'
        return dtype in (t.float32, np.float32)
    dtype = t.float32 if kind(target_mask) and kind(noise_mask) else t.float64
    return tuple(_lib.to_device(m, dtype, device=device).reshape(B, T)
                 for m in (target_mask, noise_mask))


def recursive_mvdr_souden(Y, target_mask, noise_mask, alpha=0.99, ref_channel=0,
                          initial_noise_power=1.0, *, layout=None, state=None,
                          return_state=False, return_vector=False):
    """Beamform ``Y`` frame by frame (module docstring); returns ``X (..., T)`` with the kind
    (NumPy / tensor) and dtype of ``Y``, then ``W (T, ..., D)`` complex128 with
    ``return_vector=True`` -- for ``Y (F, D, T)`` exactly what
    ``apply_online_beamforming_vector(W, Y)`` takes -- then the state with ``return_state=True``.

    ``Y``: (..., D, T), or (..., T, D) with ``layout='f t d'`` (read through its strides, nothing
    is transposed in memory); complex64 or complex128.  Masks: (..., T), float32 or float64.
    Every leading axis is an independent problem.  ``state``: an ``OnlineBeamformerState``
    returned by an earlier call, to continue its stream; it is not modified (and
    ``initial_noise_power`` is then not used).  One kernel launch; no host synchronisation for
    tensor input.  ``T = 0`` returns an empty result and leaves the state unchanged.
    """
    t = _lib.torch()
    y, like_torch = _complex_frames(Y)
    if layout is not None and layout.replace(' ', '') != 'ftd':
        raise ValueError(f"layout must be None or 'f t d', got {layout!r}")
    lead = tuple(y.shape[:-2])
    D, T = (y.shape[-2], y.shape[-1]) if layout is None else (y.shape[-1], y.shape[-2])
    B = int(np.prod(lead, dtype=np.int64))
    engine.online_bf_served(D)
    assert 0.0 < alpha <= 1.0, alpha
    assert initial_noise_power > 0.0, initial_noise_power
    assert 0 <= ref_channel < D, (ref_channel, D)
    state = (OnlineBeamformerState.initial(B, D, initial_noise_power, y.device) if state is None
             else state.clone())
    if y.numel() == 0:  # nothing to do: the state stays as it is
        x3 = t.empty((B, T), dtype=y.dtype, device=y.device)
        w3 = t.empty((T, B, D), dtype=t.complex128, device=y.device)
    else:
        s, v = _mask_rows(target_mask, noise_mask, B, T, y.device)
        x3, w3, state.status = engine.online_mvdr(
            _problems(y, layout), s, v, alpha, ref_channel, state.target_psd, state.noise_inv,
            state.frames_seen, want_vector=return_vector)
    x = x3.reshape(lead + (T,))
    out = [x if like_torch else _lib.to_host(x)]
    if return_vector:
        w = w3.reshape((T,) + lead + (D,))
        out.append(w if like_torch else _lib.to_host(w))
    if return_state:
        out.append(state)
    return out[0] if len(out) == 1 else tuple(out)


class OnlineMVDR:
    """Frame-recursive MVDR over ``frequency_bins`` bins of ``channel`` sensors, the state on the
    device: ``step_frame(frame (F, D), target_mask (F,), noise_mask (F,)) -> (F,)`` and
    ``step_block(block (F, Tb, D), target_mask (F, Tb), noise_mask (F, Tb)) -> (F, Tb)``, one
    kernel launch each, no host synchronisation for tensor input.  The shapes are those of
    ``OnlineWPE``, whose output chains into this without a transpose or a copy.

    Attributes: ``target_psd``, ``noise_inv`` (F, D, D), ``status`` (F,) int32: the status words
    of the last call, and ``vector`` (F, D): the last ``w`` (None before the first frame)."""

    def __init__(self, channel=8, frequency_bins=257, alpha=0.99, ref_channel=0,
                 initial_noise_power=1.0):
        _lib.require_gpu()
        assert 0.0 < alpha <= 1.0, alpha
        assert 0 <= ref_channel < channel, (ref_channel, channel)
        self.channel, self.frequency_bins = channel, frequency_bins
        self.alpha, self.ref_channel = alpha, ref_channel
        self.state = OnlineBeamformerState.initial(frequency_bins, channel, initial_noise_power)
        self.vector = None

    target_psd = property(lambda self: self.state.target_psd)
    noise_inv = property(lambda self: self.state.noise_inv)
    status = property(lambda self: self.state.status)

    def step_block(self, block, target_mask, noise_mask):
        """block (F, Tb, D), masks (F, Tb) -> the beamformed block (F, Tb); advances the state."""
        y, like_torch = _complex_frames(block, 'block')
        F, D = self.frequency_bins, self.channel
        assert y.ndim == 3 and y.shape[0] == F and y.shape[2] == D, (tuple(y.shape), F, D)
        Tb = y.shape[1]
        if Tb == 0:
            x = _lib.torch().empty((F, 0), dtype=y.dtype, device=y.device)
            return x if like_torch else _lib.to_host(x)
        st = self.state
        dev = st.target_psd.device
        s, v = _mask_rows(target_mask, noise_mask, F, Tb, dev)
        x, w, st.status = engine.online_mvdr(
            y.to(dev).transpose(1, 2), s, v, self.alpha, self.ref_channel, st.target_psd,
            st.noise_inv, st.frames_seen, want_vector=True)
        self.vector = w[-1]
        return x if like_torch else _lib.to_host(x)

    def step_frame(self, frame, target_mask, noise_mask):
        """frame (F, D), masks (F,) -> the beamformed frame (F,); advances the state."""
        y, like_torch = _complex_frames(frame, 'frame')
        F = self.frequency_bins
        s, v = (m.reshape(F, 1) if _lib.is_torch(m) else np.asarray(m).reshape(F, 1)
                for m in (target_mask, noise_mask))
        x = self.step_block(y.unsqueeze(1), s, v).squeeze(1)
        return x if like_torch else _lib.to_host(x)
