"""Frame-recursive (online) cACGMM mask estimator on the device: the stage between ``OnlineWPE``
and ``OnlineMVDR`` -- masks frame by frame from a complex angular central Gaussian mixture whose
class covariances are updated once per frame with exponential forgetting.

The reference only has the batch EM (``CACGMMTrainer.fit``); this docstring is the specification
(restated in NumPy by tests/oracle_online_cacgmm.py).  It is the cACG M-step of
``ComplexAngularCentralGaussianTrainer._fit`` turned into a running mean,
``B_k <- (alpha Lambda_k B_k + D gamma_k z z^H / q_k) / Lambda_k'``, with the inverse kept by
Sherman-Morrison and the determinant by the matrix determinant lemma.

For one problem (one bin) with D sensors and K classes.  State, float64 / complex128 on the
device: ``precision`` P_k (K, D, D), Hermitian, the inverse of the class covariance B_k;
``log_determinant`` L_k = log det B_k; ``count`` Lambda_k > 0, the forgotten posterior mass;
``weight`` pi_k > 0; ``frames_seen``.  Parameters: ``0 < alpha <= 1``, ``affiliation_eps >= 0``
(1e-10 as the trainer uses), ``update_weight``.  Per frame ``y``, in this order::

    nu = sqrt(sum_d |y_d|^2)
    if nu == 0:  gamma_k = pi_k, q_k = 0, the state is not touched (frames_seen advances)
    z    = y / nu                                (normalize_observation)
    n_k  = P_k z
    q_k  = Re(z^H n_k)
    lp_k = log pi_k - L_k - D log q_k            (the cACG log-pdf plus the log weight)
    gamma = softmax_k(lp), the maximum subtracted first; with affiliation_eps > 0 clipped to
            [eps, 1 - eps] and not renormalised (log_pdf_to_affiliation)
    for every k, with the gamma and q of THIS frame:
        old = alpha Lambda_k;  new = old + gamma_k;  den = old + D gamma_k
        P_k <- (P_k - ((D gamma_k / (q_k den)) n_k) n_k^H) * (new / old)
               the lower triangle is computed, the diagonal kept real, the upper triangle IS the
               conjugate mirror
        L_k <- L_k + D log(old / new) + log(den / old)
        Lambda_k <- new
    if update_weight:  pi_k = Lambda_k / sum_j Lambda_j

The masks are a-priori: the ``gamma`` of a frame does not contain that frame's own update.  The
recursion applies no eigenvalue floor and no covariance normalisation: the log-pdf does not depend
on the scale of B, and the update keeps ``tr(P D z z^H / q) = D``, so the scale does not drift.

Consequences.  After T frames, with the recorded gamma and q, ``Lambda_k = alpha^T Lambda0_k +
sum_t alpha^(T-1-t) gamma_kt``, ``B_k = (alpha^T Lambda0_k B0_k + D sum_t alpha^(T-1-t)
(gamma_kt / q_kt) z_t z_t^H) / Lambda_k``, ``P_k = B_k^-1`` and ``L_k = log det B_k``.  The first
non-zero frame's gamma and q, from a state built off a ``CACGMM``, are those of
``CACGMM.predict(..., return_quadratic_form=True)`` on that frame up to the clip.  A stream cut
into blocks of any lengths gives what one call gives, bit for bit; a batch gives bitwise what its
problems give alone; results are bit-identical from call to call.

A problem is flagged (``PBBSS_ST_NONFINITE`` in ``state.status`` / ``OnlineCACGMM.status``) when a
``q_k`` or an ``old`` is not > 0, or when a q, gamma, L or Lambda is not finite: its gamma and q
from that frame on are NaN, and so are its P, L, Lambda and pi; the other problems of the call are
unaffected.

Known limit: with ``alpha < 1`` a class that receives no mass loses its count geometrically, and
the next frame it wins then replaces its covariance by a near rank-one matrix.

Served: 2 <= D <= 16 sensors, 2 <= K <= 8 classes, any T, any number of problems; beyond that
``NotImplementedError`` names ``ONLINE_CACGMM_MAX_D = 16`` / ``ONLINE_CACGMM_MAX_K = 8``.
"""
import numpy as np

from .. import _lib, engine
from ..transform.wpe import _complex_frames, _problems

__all__ = ['recursive_cacgmm', 'OnlineCACGMM', 'OnlineCACGMMState']

INITIAL_COUNT = 10.0   # frames of posterior mass that the initial model stands for


def _shape(a):
    return tuple(a.shape)


class OnlineCACGMMState:
    """The state of a stream of B problems, on the device: ``precision`` (B, K, D, D) complex128,
    ``log_determinant``, ``count``, ``weight`` (B, K) float64, ``frames_seen`` (B,) int64;
    ``status`` (B,) int32: the status words of the call that last advanced it
    (``PBBSS_ST_NONFINITE`` for a flagged problem), None before the first one."""

    def __init__(self, precision, log_determinant, count, weight, frames_seen, status=None):
        self.precision, self.log_determinant = precision, log_determinant
        self.count, self.weight = count, weight
        self.frames_seen, self.status = frames_seen, status

    @classmethod
    def from_model(cls, model, initial_count=INITIAL_COUNT, device=None, *, lead=None):
        """From a ``CACGMM`` with parameters (..., K, D, D) / (..., K, D) and ``weight``
        (..., K, 1): ``P = V diag(1 / lambda) V^H``, ``L = sum log lambda``,
        ``pi = weight[..., 0]``, ``Lambda = initial_count * pi``.  Every leading axis is a
        problem (``lead``: the leading shape to broadcast them to).  A weight of any other
        shape raises ``ValueError``."""
        vec, val, weight = (model.cacg.covariance_eigenvectors, model.cacg.covariance_eigenvalues,
                            model.weight)
        if vec is None or val is None or weight is None:
            raise ValueError('the model has no parameters')
        if len(_shape(vec)) < 3 or _shape(vec)[-1] != _shape(vec)[-2] or \
                _shape(val) != _shape(vec)[:-1]:
            raise ValueError(f'eigenvectors (..., K, D, D) and eigenvalues (..., K, D) expected, '
                             f'got {_shape(vec)} and {_shape(val)}')
        K, D = _shape(vec)[-3:-1]
        if len(_shape(weight)) < 2 or _shape(weight)[-2:] != (K, 1):
            raise ValueError(f'only a weight of shape (..., K, 1) = (..., {K}, 1) is served, got '
                             f'{_shape(weight)}')
        if not initial_count > 0.0:
            raise ValueError(f'initial_count must be > 0, got {initial_count}')
        engine.online_cacgmm_served(D, K)
        t = _lib.require_gpu()
        if device is None:
            device = vec.device if _lib.is_torch(vec) and vec.is_cuda else \
                t.device('cuda', t.cuda.current_device())
        vec = _lib.to_device(vec, t.complex128, device=device)
        val = _lib.to_device(val, t.float64, device=device)
        pi = _lib.to_device(weight, t.float64, device=device)[..., 0]
        if lead is None:
            lead = tuple(np.broadcast_shapes(_shape(vec)[:-3], _shape(pi)[:-1]))
        B = int(np.prod(lead, dtype=np.int64))
        P = t.einsum('...de,...e,...ge->...dg', vec, (1.0 / val).to(t.complex128), vec.conj())
        P = P.expand(*lead, K, D, D).reshape(B, K, D, D).contiguous()
        L = val.log().sum(dim=-1).expand(*lead, K).reshape(B, K).contiguous()
        pi = pi.expand(*lead, K).reshape(B, K).contiguous()
        return cls(P, L, pi * initial_count, pi.clone(),
                   t.zeros((B,), dtype=t.int64, device=device))

    def clone(self):
        return OnlineCACGMMState(self.precision.clone(), self.log_determinant.clone(),
                                 self.count.clone(), self.weight.clone(),
                                 self.frames_seen.clone(), self.status)


def _parameters(alpha, affiliation_eps):
    assert 0.0 < alpha <= 1.0, alpha
    assert 0.0 <= affiliation_eps < 0.5, affiliation_eps


def recursive_cacgmm(Y, initialization=None, alpha=0.99, *, affiliation_eps=1e-10,
                     update_weight=True, initial_count=INITIAL_COUNT, layout=None, state=None,
                     return_state=False, return_quadratic_form=False):
    """Masks of ``Y`` frame by frame (module docstring); returns ``affiliation (..., K, T)``
    float64 of the kind (NumPy / tensor) of ``Y``, then ``quadratic_form (..., K, T)`` with
    ``return_quadratic_form=True``, then the state with ``return_state=True``.

    ``Y``: (..., D, T), or (..., T, D) with ``layout='f t d'`` (read through its strides, nothing
    is transposed in memory); complex64 or complex128.  Every leading axis is an independent
    problem.  Exactly one of ``initialization`` -- a ``CACGMM`` whose leading axes broadcast to
    those of ``Y``, e.g. an offline fit of a first block -- and ``state`` -- an
    ``OnlineCACGMMState`` returned by an earlier call, to continue its stream -- is given; the
    passed state is not modified.  One kernel launch; no host synchronisation for tensor input.
    ``T = 0`` returns empty results and leaves the state unchanged.
    """
    if (initialization is None) == (state is None):
        raise ValueError('exactly one of initialization and state must be given')
    if layout is not None and layout.replace(' ', '') != 'ftd':
        raise ValueError(f"layout must be None or 'f t d', got {layout!r}")
    _parameters(alpha, affiliation_eps)
    t = _lib.torch()
    y, like_torch = _complex_frames(Y)
    lead = tuple(y.shape[:-2])
    D, T = (y.shape[-2], y.shape[-1]) if layout is None else (y.shape[-1], y.shape[-2])
    B = int(np.prod(lead, dtype=np.int64))
    state = (OnlineCACGMMState.from_model(initialization, initial_count, y.device, lead=lead)
             if state is None else state.clone())
    K = state.precision.shape[1]
    engine.online_cacgmm_served(D, K)
    assert tuple(state.precision.shape) == (B, K, D, D), (tuple(state.precision.shape), B, K, D)
    if y.numel() == 0:  # nothing to do: the state stays as it is
        aff3 = t.empty((B, K, T), dtype=t.float64, device=y.device)
        q3 = t.empty((B, K, T), dtype=t.float64, device=y.device)
    else:
        aff3, q3, state.status = engine.online_cacgmm(
            _problems(y, layout), alpha, affiliation_eps, update_weight, state.precision,
            state.log_determinant, state.count, state.weight, state.frames_seen,
            want_q=return_quadratic_form)
    out = [aff3.reshape(lead + (K, T))]
    if return_quadratic_form:
        out.append(q3.reshape(lead + (K, T)))
    out = [a if like_torch else _lib.to_host(a) for a in out]
    if return_state:
        out.append(state)
    return out[0] if len(out) == 1 else tuple(out)


class OnlineCACGMM:
    """Frame-recursive cACGMM masks over the F bins of ``model`` (a ``CACGMM`` with parameters
    (F, K, D, D) / (F, K, D) and weight (F, K, 1), e.g. an offline fit of a first block, which
    also fixes the frequency permutation), the state on the device:
    ``step_frame(frame (F, D)) -> (F, K)`` and ``step_block(block (F, Tb, D)) -> (F, K, Tb)``,
    one kernel launch each, no host synchronisation for tensor input.  The shapes are those of
    ``OnlineWPE`` / ``OnlineMVDR``: the output of ``OnlineWPE.step_block`` goes in as it is, and
    ``affiliation[:, k]`` goes straight into ``OnlineMVDR.step_block`` as a mask.

    Attributes: ``precision`` (F, K, D, D), ``log_determinant``, ``count``, ``weight`` (F, K),
    ``status`` (F,) int32: the status words of the last call (None before the first one)."""

    def __init__(self, model, alpha=0.99, *, affiliation_eps=1e-10, update_weight=True,
                 initial_count=INITIAL_COUNT, device=None):
        _parameters(alpha, affiliation_eps)
        self.alpha, self.affiliation_eps = alpha, affiliation_eps
        self.update_weight = update_weight
        # an OnlineCACGMMState (copied) continues its stream
        self.state = (model.clone() if isinstance(model, OnlineCACGMMState) else
                      OnlineCACGMMState.from_model(model, initial_count, device))
        self.frequency_bins, self.num_classes, self.channel = self.state.precision.shape[:3]

    precision = property(lambda self: self.state.precision)
    log_determinant = property(lambda self: self.state.log_determinant)
    count = property(lambda self: self.state.count)
    weight = property(lambda self: self.state.weight)
    status = property(lambda self: self.state.status)

    def step_block(self, block, return_quadratic_form=False):
        """block (F, Tb, D) -> the masks (F, K, Tb) of its frames; advances the state."""
        y, like_torch = _complex_frames(block, 'block')
        F, K, D = self.frequency_bins, self.num_classes, self.channel
        assert y.ndim == 3 and y.shape[0] == F and y.shape[2] == D, (tuple(y.shape), F, D)
        st = self.state
        dev = st.precision.device
        if y.shape[1] == 0:
            out = [_lib.torch().empty((F, K, 0), dtype=_lib.torch().float64, device=dev)] * 2
        else:
            aff, q, st.status = engine.online_cacgmm(
                y.to(dev).transpose(1, 2), self.alpha, self.affiliation_eps, self.update_weight,
                st.precision, st.log_determinant, st.count, st.weight, st.frames_seen,
                want_q=return_quadratic_form)
            out = [aff, q]
        out = [a if like_torch else _lib.to_host(a) for a in out[:1 + bool(return_quadratic_form)]]
        return out[0] if len(out) == 1 else tuple(out)

    def step_frame(self, frame, return_quadratic_form=False):
        """frame (F, D) -> the masks (F, K) of that frame; advances the state."""
        y, like_torch = _complex_frames(frame, 'frame')
        out = self.step_block(y.unsqueeze(1), return_quadratic_form)
        out = [a.squeeze(2) for a in (out if return_quadratic_form else (out,))]
        out = [a if like_torch else _lib.to_host(a) for a in out]
        return out[0] if len(out) == 1 else tuple(out)
