"""Thin device-tensor layer over the C ABI for the mixture models, the beamformers, permutation
alignment and the STFT (the masks, the evaluation metrics, k-means and the gammatone filterbank
bind their exports in their own modules): every function takes/returns contiguous torch CUDA
tensors with the independent axes flattened to one batch axis B, launches exactly the library
call named in its docstring on the current torch stream, and raises the reference's exception
types from status words.

No arithmetic is done here beyond shape bookkeeping, and no marshalling either: handle, stream,
pointers, scalar conversion and the return-code check are `_lib.launch` / `_lib.control`.
"""
import ctypes
import os
import threading

import numpy as np

from . import _lib


def _t():
    return _lib.torch()


# launch(..., accept=_NOT_SERVED): PBBSS_ERR_UNSUPPORTED is an answer of the call, not an error
_NOT_SERVED = (_lib.ERR_UNSUPPORTED,)


def _status_bits(status):
    """OR of all status words (one small D2H copy; 0 without it when every word is 0)."""
    if not status.numel() or int(status.max().item()) == 0:
        return 0
    return int(np.bitwise_or.reduce(_lib.to_host(status).ravel()))


class StatusAssertionError(AssertionError):
    """The reference's `assert np.isfinite(...)` failure, derived from a kernel's status words
    (an AssertionError for callers that catch the reference's; a type of its own for callers that
    must tell a status failure from an argument check)."""


class StatusLinAlgError(np.linalg.LinAlgError):
    """The reference's eigensolver failure, derived from a kernel's status words."""


def _raise_for_bits(bits, what):
    """Mirror the reference's failure modes of the M-step."""
    if bits & _lib.ST_NONFINITE:
        # distribution/complex_angular_central_gaussian.py:127, :326, :333
        raise StatusAssertionError(
            f'{what}: non-finite covariance / eigenvalues '
            '(reference: assert np.isfinite(...))')
    if bits & _lib.ST_EIG_NOCONV:
        # complex_angular_central_gaussian.py:94-110 (LinAlgError from eigh/eig)
        raise StatusLinAlgError(f'{what}: Hermitian eigensolver did not converge')
    if bits & _lib.ST_SOLVE_NOCONV:
        # complex_bingham.py:376-383 (only the complex Bingham kernels set this bit)
        raise StatusLinAlgError(f'{what}: complex Bingham parameter solve did not converge')


def _status_raise_em(status, what):
    _raise_for_bits(_status_bits(status), what)


_SPLIT_POISON = _lib.ST_NONFINITE | _lib.ST_EIG_NOCONV


def _checked_with_split_retry(launch, dev, what):
    """Run launch() -> dict with 'status' and raise for its status bits.  The split groups of a
    remainder bin (2^n + 1 bins) exchange their sums through bounded waits; when one runs out
    -- the member workgroups were not on the chip together: compute units held by other work --
    the launch marks the problems concerned with NONFINITE | EIG_NOCONV and raises the flag of
    pbbss_split_error.  That is not a numerical failure: repeat once without split groups."""
    r = launch()
    bits = _status_bits(r['status'])
    if (bits & _SPLIT_POISON) == _SPLIT_POISON and split_error(dev.index):
        import warnings
        warnings.warn(f'{what}: the split groups of the remainder bin were not co-resident (GPU '
                      'shared with other work); repeating the fit without them', RuntimeWarning)
        # consume the report: counters and the sticky flag go back to zero, so that a later
        # genuine NONFINITE | EIG_NOCONV failure of this handle is raised, not refitted
        split_reset(dev.index)
        was = split_tail(dev.index)
        set_split_tail(False, dev.index)
        try:
            r = launch()
            bits = _status_bits(r['status'])
        finally:
            set_split_tail(was, dev.index)  # what the caller had chosen, not unconditionally on
    _raise_for_bits(bits, what)
    return r


def _cooperative_timed_out(status, dev):
    """True when a cooperative shared-weight launch did not get its workgroups co-resident (other
    kernels of this process held the compute units): some status words carry the time-out pattern
    -- .any(): the groups of a big batch go out as several cooperative launches, one of which can
    time out alone -- and the handle's wait flag is up.  Not a numerical failure: the report is
    consumed (see _checked_with_split_retry), the caller of the engine function is warned and the
    function answers "not served", so that the step-wise loop, which needs no co-residency, runs."""
    # the status test first: split_error() is a blocking read of the handle's flag word and is
    # only worth its round trip when some status word carries the time-out pattern
    if not (bool(((status & _SPLIT_POISON) == _SPLIT_POISON).any().item())
            and split_error(dev.index)):
        return False
    import warnings
    warnings.warn('cooperative shared-weight launch timed out waiting for co-residency; '
                  'repeating the fit step by step', RuntimeWarning, stacklevel=3)
    split_reset(dev.index)
    return True


def normalize_observation(y):
    """pbbss_normalize_observation: (B,T,D) complex -> (B,D,T), unit norm."""
    t = _t()
    B, T, D = y.shape
    is128 = y.dtype == t.complex128
    out = t.empty((B, D, T), dtype=y.dtype, device=y.device)
    _lib.launch('pbbss_normalize_observation', y.device, y, is128, B, T, D, out,
                what='normalize_observation')
    return out


def _btd(y, layout):
    """(B, T, D) of an observation in `layout`"""
    if layout == _lib.LAYOUT_TD:
        B, T, D = y.shape
    else:
        B, D, T = y.shape
    return B, T, D


def _check_em_inputs(t, model, gamma0, saliency, activity, B, K, T):
    """gamma0 (read only without a start model), saliency and activity of the cACGMM fits"""
    if model is None:
        assert gamma0.shape == (B, K, T) and gamma0.dtype == t.float64, (gamma0.shape, gamma0.dtype)
    if saliency is not None:
        assert saliency.shape == (B, T) and saliency.dtype == t.float64
    if activity is not None:
        assert activity.shape == (B, K, T) and activity.dtype == t.uint8


def em_fit(y, K, *, gamma0=None, model=None, iterations=100, saliency=None,
           activity=None, covariance_norm='eigenvalue', weight_mode=0,
           affiliation_eps=1e-10, eigenvalue_floor=1e-10, hermitize=True,
           layout=_lib.LAYOUT_TD, final_predict=False, return_q=False,
           force_eig=False, check_status=True, precision='f64'):
    """pbbss_cacgmm_fit.  y (B,T,D) [layout TD] or (B,D,T) [layout DT] complex.
    precision 'f32': the packed-FP32 "reference precision" kernel (complex64 y, D <= 8, K <= 6,
    LDS-resident frames) -- NotImplementedError where it does not apply.

    gamma0 (B,K,T) f64, or model=(eigvec (B,K,D,D) c128, eigval (B,K,D), weight (B,K)).
    Returns dict(eigvec, eigval, weight (B,K), status, affiliation?, quadratic_form?).
    """
    t = _t()
    dev = y.device
    B, T, D = _btd(y, layout)
    is128 = y.dtype == t.complex128
    assert y.dtype in (t.complex64, t.complex128), y.dtype
    opts = _lib.EmOpts(
        iterations=int(iterations),
        covariance_norm=_lib.COVNORM[covariance_norm],
        weight_mode=int(weight_mode), hermitize=int(bool(hermitize)),
        layout=int(layout), y_is_c128=int(is128),
        final_predict=int(bool(final_predict)), force_eig=int(bool(force_eig)),
        affiliation_eps=float(affiliation_eps),
        eigenvalue_floor=float(eigenvalue_floor), precision=_lib.PRECISION[precision])
    f64 = t.float64
    if model is not None:
        in_vec, in_val, in_w = model
        assert in_vec.shape == (B, K, D, D) and in_val.shape == (B, K, D) and in_w.shape == (B, K)
    else:
        in_vec = in_val = in_w = None
    _check_em_inputs(t, model, gamma0, saliency, activity, B, K, T)

    def launch():
        out_vec = t.empty((B, K, D, D), dtype=t.complex128, device=dev)
        out_val = t.empty((B, K, D), dtype=f64, device=dev)
        out_w = t.empty((B, K), dtype=f64, device=dev)
        out_st = t.empty((B, K), dtype=t.int32, device=dev)  # every row is written by the library
        out_aff = t.empty((B, K, T), dtype=f64, device=dev) if final_predict else None
        out_q = t.empty((B, K, T), dtype=f64, device=dev) if (final_predict and return_q) else None
        _lib.launch('pbbss_cacgmm_fit', dev, y, B, T, D, K, gamma0, in_vec, in_val, in_w,
                    saliency, activity, opts, out_vec, out_val, out_w, out_st, out_aff, out_q,
                    what=f'cacgmm_fit(B={B},T={T},D={D},K={K})')
        return dict(eigvec=out_vec, eigval=out_val, weight=out_w, status=out_st,
                    affiliation=out_aff, quadratic_form=out_q)

    if check_status:
        return _checked_with_split_retry(launch, dev, 'CACGMMTrainer.fit')
    return launch()


def em_fit_shared(y, K, group, *, weight_mode, gamma0=None, model=None, iterations=100,
                  saliency=None, activity=None, covariance_norm='eigenvalue',
                  affiliation_eps=1e-10, eigenvalue_floor=1e-10, final_predict=False,
                  return_q=False, force_eig=False, check_status=True):
    """pbbss_cacgmm_fit_shared: the EM loop with mixture weights estimated over `group`
    consecutive problems (weight_constant_axis (-3,) -> WEIGHT_SHARED_KT, (-3, -1) ->
    WEIGHT_SHARED_K), one cooperative launch.  y (B,T,D) complex, B = n_groups * group.
    model = (eigvec (B,K,D,D), eigval (B,K,D), weight (B/group, K[, T])).
    Returns None when the configuration is not served by the cooperative kernel
    (PBBSS_ERR_UNSUPPORTED: too many bins to be co-resident, K > 4, long utterances);
    otherwise dict(eigvec, eigval, weight (B/group, K[, T]), status, affiliation?, ...)."""
    t = _t()
    dev = y.device
    B, T, D = y.shape
    assert B % group == 0, (B, group)
    G = B // group
    is128 = y.dtype == t.complex128
    assert y.dtype in (t.complex64, t.complex128), y.dtype
    assert weight_mode in (_lib.WEIGHT_SHARED_K, _lib.WEIGHT_SHARED_KT), weight_mode
    wshape = (G, K) if weight_mode == _lib.WEIGHT_SHARED_K else (G, K, T)
    opts = _lib.EmOpts(
        iterations=int(iterations), covariance_norm=_lib.COVNORM[covariance_norm],
        weight_mode=int(weight_mode), hermitize=1, layout=int(_lib.LAYOUT_TD),
        y_is_c128=int(is128), final_predict=int(bool(final_predict)),
        force_eig=int(bool(force_eig)), affiliation_eps=float(affiliation_eps),
        eigenvalue_floor=float(eigenvalue_floor))
    f64 = t.float64
    out_vec = t.empty((B, K, D, D), dtype=t.complex128, device=dev)
    out_val = t.empty((B, K, D), dtype=f64, device=dev)
    out_w = t.empty(wshape, dtype=f64, device=dev)
    out_st = t.zeros((B, K), dtype=t.int32, device=dev)
    out_aff = t.empty((B, K, T), dtype=f64, device=dev) if final_predict else None
    out_q = t.empty((B, K, T), dtype=f64, device=dev) if (final_predict and return_q) else None
    if model is not None:
        in_vec, in_val, in_w = model
        assert in_vec.shape == (B, K, D, D) and in_val.shape == (B, K, D), in_vec.shape
        assert tuple(in_w.shape) == wshape and in_w.is_contiguous(), (in_w.shape, wshape)
    else:
        in_vec = in_val = in_w = None
    _check_em_inputs(t, model, gamma0, saliency, activity, B, K, T)
    rc = _lib.launch('pbbss_cacgmm_fit_shared', dev, y, B, T, D, K, group, gamma0, in_vec, in_val,
                     in_w, saliency, activity, opts, out_vec, out_val, out_w, out_st, out_aff,
                     out_q, what=f'cacgmm_fit_shared(B={B},group={group},T={T},D={D},K={K})',
                     accept=_NOT_SERVED)
    if rc == _lib.ERR_UNSUPPORTED:
        return None
    if check_status:
        if iterations > 0 and _cooperative_timed_out(out_st, dev):
            return None
        _status_raise_em(out_st, 'CACGMMTrainer.fit')
    return dict(eigvec=out_vec, eigval=out_val, weight=out_w, status=out_st,
                affiliation=out_aff, quadratic_form=out_q)


def em_predict(y, eigvec, eigval, weight, *, activity=None,
               layout=_lib.LAYOUT_TD, affiliation_eps=0.0,
               want_q=False, want_log_pdf=False, want_affiliation=True):
    """pbbss_cacgmm_predict.  weight is (B,K) or (B,K,T) f64."""
    t = _t()
    dev = y.device
    B, T, D = _btd(y, layout)
    K = eigvec.shape[1]
    is128 = y.dtype == t.complex128
    f64 = t.float64
    if weight.dim() == 2:
        wb, wk, wt = K, 1, 0
    else:
        assert weight.shape == (B, K, T), weight.shape
        wb, wk, wt = K * T, T, 1
    aff = t.empty((B, K, T), dtype=f64, device=dev) if want_affiliation else None
    q = t.empty((B, K, T), dtype=f64, device=dev) if want_q else None
    lp = t.empty((B, K, T), dtype=f64, device=dev) if want_log_pdf else None
    _lib.launch('pbbss_cacgmm_predict', dev, y, B, T, D, K, eigvec, eigval, weight, wb, wk, wt,
                activity, layout, is128, affiliation_eps, aff, q, lp,
                what=f'cacgmm_predict(B={B},T={T},D={D},K={K})')
    return aff, q, lp


def cacg_m_step(y, saliency, quadratic_form, *, layout=_lib.LAYOUT_DT,
                covariance_norm='eigenvalue', eigenvalue_floor=1e-10,
                want_cov=False, check_status=True):
    """pbbss_cacg_m_step: saliency/quadratic_form (B,K,T) f64."""
    t = _t()
    dev = y.device
    B, T, D = _btd(y, layout)
    K = saliency.shape[1]
    is128 = y.dtype == t.complex128

    def launch():
        out_vec = t.empty((B, K, D, D), dtype=t.complex128, device=dev)
        out_val = t.empty((B, K, D), dtype=t.float64, device=dev)
        out_st = t.zeros((B, K), dtype=t.int32, device=dev)
        out_cov = t.empty((B, K, D, D), dtype=t.complex128, device=dev) if want_cov else None
        _lib.launch('pbbss_cacg_m_step', dev, y, B, T, D, K, saliency, quadratic_form, layout,
                    is128, _lib.COVNORM[covariance_norm], eigenvalue_floor, out_vec, out_val,
                    out_cov, out_st, what=f'cacg_m_step(B={B},T={T},D={D},K={K})')
        return dict(eigvec=out_vec, eigval=out_val, cov=out_cov, status=out_st)

    # ONE iteration of the EM kernel: split groups need kSplitMinIterations = 3 (em_launch.hpp), so
    # this launch has no inter-workgroup wait and no time-out to recover from
    r = launch()
    if check_status:
        _status_raise_em(r['status'], 'ComplexAngularCentralGaussianTrainer._fit')
    return r['eigvec'], r['eigval'], r['cov'], r['status']


def heev(a):
    """pbbss_heev_batched: a (N,D,D) c128 -> (eigval (N,D), eigvec (N,D,D), status)."""
    t = _t()
    N, D, _ = a.shape
    val = t.empty((N, D), dtype=t.float64, device=a.device)
    vec = t.empty((N, D, D), dtype=t.complex128, device=a.device)
    st = t.zeros((N,), dtype=t.int32, device=a.device)
    _lib.launch('pbbss_heev_batched', a.device, a, N, D, val, vec, st, what=f'heev(N={N},D={D})')
    return val, vec, st


def psd(x, mask, normalize=True):
    """pbbss_psd: x (B,D,T) complex, mask (B,K,T) f64 or None -> (B,K,D,D) c128."""
    t = _t()
    B, D, T = x.shape
    K = 1 if mask is None else mask.shape[1]
    out = t.empty((B, K, D, D), dtype=t.complex128, device=x.device)
    _lib.launch('pbbss_psd', x.device, x, x.dtype == t.complex128, B, T, D, K, mask,
                bool(normalize), out, what=f'psd(B={B},T={T},D={D},K={K})')
    return out


def gev(target, noise):
    """pbbss_gev: (N,D,D) c128 x2 -> (w (N,D) c128, status (N,))."""
    t = _t()
    N, D, _ = target.shape
    w = t.empty((N, D), dtype=t.complex128, device=target.device)
    st = t.zeros((N,), dtype=t.int32, device=target.device)
    _lib.launch('pbbss_gev', target.device, target, noise, N, D, w, st, what=f'gev(N={N},D={D})')
    return w, st


def gev_general(target, noise, want_eigenvalue=False):
    """pbbss_gev_general: (N,D,D) c128 x2, no Hermitian assumption -> (w (N,D) unit norm,
    eigenvalue (N,) c128 or None, status (N,))."""
    t = _t()
    N, D, _ = target.shape
    w = t.empty((N, D), dtype=t.complex128, device=target.device)
    lam = t.empty((N,), dtype=t.complex128, device=target.device) if want_eigenvalue else None
    st = t.zeros((N,), dtype=t.int32, device=target.device)
    _lib.launch('pbbss_gev_general', target.device, target, noise, N, D, w, lam, st,
                what=f'gev_general(N={N},D={D})')
    return w, lam, st


def solve(A, Bm):
    """pbbss_solve: A (N,D,D), Bm (N,D,M) c128 -> (X, status)."""
    t = _t()
    N, D, _ = A.shape
    M = Bm.shape[-1]
    x = t.empty((N, D, M), dtype=t.complex128, device=A.device)
    st = t.zeros((N,), dtype=t.int32, device=A.device)
    _lib.launch('pbbss_solve', A.device, A, Bm, N, D, M, x, st, what=f'solve(N={N},D={D},M={M})')
    return x, st


def mvdr_souden(target, noise, eps):
    """pbbss_mvdr_souden -> (mat (N,D,D), snr_num (N,D), snr_den (N,D), status)."""
    t = _t()
    N, D, _ = target.shape
    mat = t.empty((N, D, D), dtype=t.complex128, device=target.device)
    num = t.empty((N, D), dtype=t.complex128, device=target.device)
    den = t.empty((N, D), dtype=t.complex128, device=target.device)
    # the fused kernels (D <= 8) write every status word; no fill launch in front of them
    st = (t.empty if D <= 8 else t.zeros)((N,), dtype=t.int32, device=target.device)
    _lib.launch('pbbss_mvdr_souden', target.device, target, noise, N, D, eps, mat, num, den, st,
                what=f'mvdr_souden(N={N},D={D})')
    return mat, num, den, st


def select_reference_channel(mat, num, den, L, F, eps, lead_stride=None, bin_stride=1):
    """pbbss_select_reference_channel (round 6): the automatic reference channel of
    get_mvdr_vector_souden (beamformer.py:601-624) and the column select (:690-698) for L problems
    of F bins in ONE launch, from the outputs of `mvdr_souden` (mat (N,D,D), num / den (N,D) c128;
    problem l, bin f = matrix l * lead_stride + f * bin_stride).
    -> (w (L,F,D) c128, ref (L) int32, ok (L) int32: every SNR of the problem finite)."""
    t = _t()
    D = mat.shape[-1]
    w = t.empty((L, F, D), dtype=t.complex128, device=mat.device)
    ref = t.empty((L,), dtype=t.int32, device=mat.device)
    ok = t.empty((L,), dtype=t.int32, device=mat.device)
    _lib.launch('pbbss_select_reference_channel', mat.device, mat, num, den, L, F, D,
                F if lead_stride is None else lead_stride, bin_stride, eps, w, ref, ok,
                what=f'select_reference_channel(L={L},F={F},D={D})')
    return w, ref, ok


def mvdr(atf, noise):
    """pbbss_mvdr: atf (N,D), noise (N,D,D) c128 -> (w (N,D), status)."""
    t = _t()
    N, D = atf.shape
    w = t.empty((N, D), dtype=t.complex128, device=atf.device)
    st = t.zeros((N,), dtype=t.int32, device=atf.device)
    _lib.launch('pbbss_mvdr', atf.device, atf, noise, N, D, w, st, what=f'mvdr(N={N},D={D})')
    return w, st


def ban(w, noise):
    """pbbss_ban: w (N,D), noise (N,D,D) c128 -> (N,D) c128."""
    t = _t()
    N, D = w.shape
    out = t.empty((N, D), dtype=t.complex128, device=w.device)
    _lib.launch('pbbss_ban', w.device, w, noise, N, D, out, what=f'ban(N={N},D={D})')
    return out


def apply_bf(w, x):
    """pbbss_apply_beamforming_vector: w (B,D) c128, x (B,D,T) -> (B,T) c128.  With fewer
    observations than vectors (x (Bx,D,T), B a multiple of Bx) problem b reads x[b % Bx] --
    pbbss_apply_beamforming_vector_shared, no copies of x."""
    t = _t()
    Bx, D, T = x.shape
    B = w.shape[0]
    out = t.empty((B, T), dtype=t.complex128, device=x.device)
    what = f'apply_beamforming_vector(B={B},Bx={Bx},T={T},D={D})'
    if B == Bx:
        _lib.launch('pbbss_apply_beamforming_vector', x.device, w, x, x.dtype == t.complex128,
                    B, T, D, out, what=what)
    else:
        _lib.launch('pbbss_apply_beamforming_vector_shared', x.device, w, x,
                    x.dtype == t.complex128, B, Bx, T, D, out, what=what)
    return out


def set_timing(enable, device_index=None):
    _lib.control('pbbss_set_timing', device_index, enable, what='set_timing')


def last_kernel_ms(device_index=None, lag=0):
    """Duration of the timed region `lag` launches ago (0 = the most recent: waits for it).  Read
    with lag = 2 inside a loop of launches, the queue keeps two launches behind the running one
    (pbbss_kernel_ms_lagged)."""
    ms = ctypes.c_float()
    _lib.control('pbbss_kernel_ms_lagged', device_index, lag, ms, what='kernel_ms_lagged')
    return float(ms.value)


PA_METRIC = {'cos': 0, 'multiply': 1, 'euclidean': 2}


def dhtv_calculate_mapping(mask, plan, optimal=False, metric='cos'):
    """pbbss_dhtv_calculate_mapping: mask (U,K,F,T) f64, plan int32 (P,3) on the
    device -> (mapping int32 (U,K,F), aligned unit-norm features (U,K,F,T), status (U,))."""
    t = _t()
    U, K, F, T = mask.shape
    feat = t.empty_like(mask)
    mapping = t.empty((U, K, F), dtype=t.int32, device=mask.device)
    st = t.zeros((U,), dtype=t.int32, device=mask.device)
    _lib.launch('pbbss_dhtv_calculate_mapping', mask.device, mask, U, K, F, T, plan,
                plan.shape[0], bool(optimal), PA_METRIC[metric], feat, mapping, st,
                what=f'dhtv_calculate_mapping(U={U},K={K},F={F},T={T})')
    return mapping, feat, st


def apply_mapping(mask, mapping):
    """pbbss_apply_mapping: mask (U,K,F,T) f64, mapping int32 (U,K,F) -> (U,K,F,T)."""
    t = _t()
    U, K, F, T = mask.shape
    out = t.empty_like(mask)
    _lib.launch('pbbss_apply_mapping', mask.device, mask, mapping, U, K, F, T, out,
                what=f'apply_mapping(U={U},K={K},F={F},T={T})')
    return out


def _strides3(x):
    """element strides of (utterance, class, bin) of a (U,K,F,T) tensor with contiguous frames"""
    assert x.stride(-1) == 1 or x.shape[-1] == 1, x.stride()
    return (ctypes.c_int64 * 3)(x.stride(0), x.stride(1), x.stride(2))


def pa_pairwise_mapping(mask, reference, metric, optimal, *, mapping=None, col0=0,
                        want_scores=False):
    """pbbss_pa_pairwise_mapping: mask / reference (U,K,F,T) f64 views (frames contiguous)
    -> (mapping int32 (U,K,map_F) with columns col0 .. col0+F-1 filled, scores or None,
    status (U,))."""
    t = _t()
    U, K, F, T = mask.shape
    assert tuple(reference.shape) == (U, K, F, T), (mask.shape, reference.shape)
    if mapping is None:
        mapping = t.empty((U, K, col0 + F), dtype=t.int32, device=mask.device)
    scores = t.empty((U, F, K, K), dtype=t.float64, device=mask.device) if want_scores else None
    st = t.zeros((U,), dtype=t.int32, device=mask.device)
    _lib.launch('pbbss_pa_pairwise_mapping', mask.device, _lib.view_ptr(mask),
                _lib.view_ptr(reference), U, K, F, T, _strides3(mask), _strides3(reference),
                PA_METRIC[metric], bool(optimal), scores, mapping, mapping.shape[-1], col0, st,
                what=f'pa_pairwise_mapping(U={U},K={K},F={F},T={T},{metric})')
    return mapping, scores, st


def pa_compose_mapping(mapping):
    """pbbss_pa_compose_mapping, in place on mapping int32 (U,K,F)."""
    U, K, F = mapping.shape
    _lib.launch('pbbss_pa_compose_mapping', mapping.device, mapping, U, K, F,
                what=f'pa_compose_mapping(U={U},K={K},F={F})')
    return mapping


def pa_mapping_from_scores(scores, optimal):
    """pbbss_pa_mapping_from_scores: scores (N,K,K) f64 -> (mapping int32 (K,N), status (1,))."""
    t = _t()
    N, K, _ = scores.shape
    mapping = t.empty((K, N), dtype=t.int32, device=scores.device)
    st = t.zeros((1,), dtype=t.int32, device=scores.device)
    _lib.launch('pbbss_pa_mapping_from_scores', scores.device, scores, N, K, bool(optimal),
                mapping, st, what=f'pa_mapping_from_scores(N={N},K={K})')
    return mapping, st


def cwmm_fit(y, K, spline, *, gamma0=None, model=None, iterations=100, saliency=None,
             weight_mode=0, final_predict=False, want_log_pdf=False, check_status=True,
             group=None):
    """pbbss_cwmm_fit.  y (B,T,D) complex; gamma0 (B,K,T) f64 or
    model=(mode (B,K,D) c128, concentration (B,K), weight (B,K)).
    `spline` = dict(t, c device f64 arrays, ev_min, ev_max, max_concentration);
    may be None for a pure predict (iterations=0).
    group (with weight_mode=_lib.WEIGHT_SHARED_K): consecutive problems that share one weight
    set (weight_constant_axis (-3, -1)); the weight comes back as (B / group, K).  Returns None
    when the cooperative kernel does not serve the configuration or its grid barrier timed out
    (a RuntimeWarning): the caller then runs the loop step by step."""
    t = _t()
    dev = y.device
    B, T, D = y.shape
    is128 = y.dtype == t.complex128
    shared = weight_mode in (_lib.WEIGHT_SHARED_K, _lib.WEIGHT_SHARED_KT)
    opts = _lib.CwmmOpts(
        iterations=int(iterations), weight_mode=int(weight_mode), y_is_c128=int(is128),
        final_predict=int(bool(final_predict or want_log_pdf)),
        n_coef=0 if spline is None else int(spline['c'].numel()),
        group=int(group) if shared else 0,
        ev_min=0.0 if spline is None else float(spline['ev_min']),
        ev_max=0.0 if spline is None else float(spline['ev_max']),
        max_concentration=0.0 if spline is None else float(spline['max_concentration']))
    f64 = t.float64
    in_mode = in_conc = in_w = None
    if model is not None:
        in_mode, in_conc, in_w = model
        assert in_mode.shape == (B, K, D) and in_conc.shape == (B, K) and in_w.shape == (B, K)
    else:
        assert gamma0.shape == (B, K, T) and gamma0.dtype == f64

    def launch():
        out_mode = t.empty((B, K, D), dtype=t.complex128, device=dev)
        out_conc = t.empty((B, K), dtype=f64, device=dev)
        out_w = t.empty(((B // group, K, T) if weight_mode == _lib.WEIGHT_SHARED_KT else
                         (B // group, K)) if shared else (B, K), dtype=f64, device=dev)
        out_st = t.zeros((B, K), dtype=t.int32, device=dev)
        out_aff = t.empty((B, K, T), dtype=f64, device=dev) if final_predict else None
        out_lp = t.empty((B, K, T), dtype=f64, device=dev) if want_log_pdf else None
        rc = _lib.launch('pbbss_cwmm_fit', dev, y, B, T, D, K, gamma0, in_mode, in_conc, in_w,
                         saliency, opts, None if spline is None else spline['t'],
                         None if spline is None else spline['c'], out_mode, out_conc, out_w,
                         out_st, out_aff, out_lp, what=f'cwmm_fit(B={B},T={T},D={D},K={K})',
                         accept=_NOT_SERVED if shared else ())
        if rc == _lib.ERR_UNSUPPORTED:
            return None
        return dict(mode=out_mode, concentration=out_conc, weight=out_w, status=out_st,
                    affiliation=out_aff, log_pdf=out_lp)

    if shared:
        r = launch()
        if r is None:
            return None
        if check_status:
            if _cooperative_timed_out(r['status'], dev):
                return None
            _status_raise_em(r['status'], 'CWMMTrainer.fit')
        return r
    if check_status and iterations > 0:
        return _checked_with_split_retry(launch, dev, 'CWMMTrainer.fit')
    return launch()


def cbmm_fit(y, K, *, gamma0=None, model=None, iterations=100, saliency=None, weight_mode=0,
             max_concentration=float('inf'), eigenvalue_eps=1e-8, norm_eps=1e-8, final_predict=False,
             want_log_pdf=False, check_status=True):
    """pbbss_cbmm_fit.  y (B,T,D) complex; gamma0 (B,K,T) f64 or
    model=(eigvec (B,K,D,D) c128, eigval (B,K,D) f64, weight (B,K) f64).  norm_eps: the
    de-duplication spacing of ln c (ComplexBingham.norm's eps; 0 keeps the eigenvalues)."""
    t = _t()
    dev = y.device
    B, T, D = y.shape
    f64 = t.float64
    opts = _lib.CbmmOpts(
        iterations=int(iterations), weight_mode=int(weight_mode),
        y_is_c128=int(y.dtype == t.complex128),
        final_predict=int(bool(final_predict or want_log_pdf)),
        max_concentration=float(max_concentration), eigenvalue_eps=float(eigenvalue_eps),
        norm_eps=float(norm_eps))
    in_v = in_l = in_w = None
    if model is not None:
        in_v, in_l, in_w = model
        assert in_v.shape == (B, K, D, D) and in_l.shape == (B, K, D) and in_w.shape == (B, K)
    else:
        assert gamma0.shape == (B, K, T) and gamma0.dtype == f64
    out_v = t.empty((B, K, D, D), dtype=t.complex128, device=dev)
    out_l = t.empty((B, K, D), dtype=f64, device=dev)
    out_c = t.empty((B, K), dtype=f64, device=dev)
    out_w = t.empty((B, K), dtype=f64, device=dev)
    out_st = t.zeros((B, K), dtype=t.int32, device=dev)
    out_aff = t.empty((B, K, T), dtype=f64, device=dev) if final_predict else None
    out_lp = t.empty((B, K, T), dtype=f64, device=dev) if want_log_pdf else None
    _lib.launch('pbbss_cbmm_fit', dev, y, B, T, D, K, gamma0, in_v, in_l, in_w, saliency, opts,
                out_v, out_l, out_c, out_w, out_st, out_aff, out_lp,
                what=f'cbmm_fit(B={B},T={T},D={D},K={K})')
    if check_status:
        _status_raise_em(out_st, 'CBMMTrainer.fit')
    return dict(eigvec=out_v, eigval=out_l, log_norm=out_c, weight=out_w, status=out_st,
                affiliation=out_aff, log_pdf=out_lp)


def cbingham_find_eigenvalues(scatter, eigenvalue_eps=1e-8, max_concentration=float('inf'),
                              check_status=True):
    """pbbss_cbingham_find_eigenvalues.  scatter (N,D) f64 device -> (lam (N,D), status (N,))."""
    t = _t()
    dev = scatter.device
    N, D = scatter.shape
    lam = t.empty((N, D), dtype=t.float64, device=dev)
    st = t.zeros((N,), dtype=t.int32, device=dev)
    _lib.launch('pbbss_cbingham_find_eigenvalues', dev, scatter, N, D, eigenvalue_eps,
                max_concentration, lam, st, what=f'cbingham_find_eigenvalues(N={N},D={D})')
    if check_status:
        _status_raise_em(st, 'ComplexBinghamTrainer.find_eigenvalues_v3')
    return lam, st


def deflation_seed(y, K, *, saliency=None, permutation_free=True, neighbors=5, eps=0.0,
                   rounds=None, finalize=True, state=None, out=None, want_peak=False):
    """pbbss_deflation_seed.  y (B,F,T,D) complex -> posterior (B,K,F,T) f64 (and the peak frames
    (B,K-1,F) int32 with want_peak).  rounds=(begin, end) with `state` (B,F,T) and `out` runs a
    part of the K - 1 deflation rounds (similarity_transform path); default: the whole seed."""
    t = _t()
    dev = y.device
    B, F, T, D = y.shape
    r0, r1 = (0, K - 1) if rounds is None else rounds
    if out is None:
        out = t.empty((B, K, F, T), dtype=t.float64, device=dev)
    assert out.shape == (B, K, F, T) and out.dtype == t.float64
    assert saliency is None or (saliency.shape == (B, F, T) and saliency.dtype == t.float64)
    assert state is None or (state.shape == (B, F, T) and state.dtype == t.float64)
    peak = t.empty((B, K - 1, F), dtype=t.int32, device=dev) if want_peak else None
    _lib.launch('pbbss_deflation_seed', dev, y, y.dtype == t.complex128, B, F, T, D, K, saliency,
                bool(permutation_free), neighbors, eps, r0, r1, bool(finalize), state, out, peak,
                what=f'deflation_seed(B={B},F={F},T={T},D={D},K={K})')
    return (out, peak) if want_peak else out


def wmwf(target, noise, distortion_weight=1.0, frequency_dependent=False):
    """pbbss_wmwf -> (filter matrix (N,D,D), snr_num (N,D), snr_den (N,D), status)."""
    t = _t()
    N, D, _ = target.shape
    mat = t.empty((N, D, D), dtype=t.complex128, device=target.device)
    num = t.empty((N, D), dtype=t.complex128, device=target.device)
    den = t.empty((N, D), dtype=t.complex128, device=target.device)
    st = t.zeros((N,), dtype=t.int32, device=target.device)
    _lib.launch('pbbss_wmwf', target.device, target, noise, N, D, distortion_weight,
                bool(frequency_dependent), mat, num, den, st, what=f'wmwf(N={N},D={D})')
    return mat, num, den, st


# (device index, host thread) -- one C handle each -- -> {'split_tail' | 'dhtv_team' |
# 'dhtv_probe': the value this layer last set}; a getter without an entry answers the default
# the library creates the handle with
_SETTINGS = {}


def _handle_key(device_index):
    if device_index is None:
        device_index = _lib.require_gpu().cuda.current_device()
    return (device_index, threading.get_ident())


def _settings(device_index):
    return _SETTINGS.setdefault(_handle_key(device_index), {})


def set_split_tail(enable, device_index=None):
    """pbbss_set_split_tail: toggle the split-bin handling of remainder problems."""
    _lib.control('pbbss_set_split_tail', device_index, bool(enable), what='set_split_tail')
    _settings(device_index)['split_tail'] = bool(enable)


def split_tail(device_index=None):
    """The split-tail setting in force on this thread's handle (handles are created with it on)."""
    return _settings(device_index).get('split_tail', True)


def set_spin_limit(polls, device_index=None):
    """pbbss_set_spin_limit (test knob): polls before a bounded inter-workgroup wait gives up;
    0 = defaults.  A tiny value provokes real time-outs of the split / team protocols."""
    _lib.control('pbbss_set_spin_limit', device_index, polls, what='set_spin_limit')


def split_reset(device_index=None):
    """pbbss_split_reset: consume a reported time-out (re-zero the protocol counters and the
    sticky flag of split_error) after the device has drained."""
    _lib.control('pbbss_split_reset', device_index, what='split_reset')


def split_error(device_index=None):
    """pbbss_split_error: 1 if an inter-workgroup wait of a split launch ever timed out."""
    flag = ctypes.c_int()
    _lib.control('pbbss_split_error', device_index, flag, what='split_error')
    return int(flag.value)


def set_dhtv_team(workgroups_per_utterance, device_index=None):
    """pbbss_set_dhtv_team: 0 automatic, 1 one workgroup per utterance, >= 2 frame-slice kernel,
    -2..-32 bin-chunk team kernel of that size."""
    _lib.control('pbbss_set_dhtv_team', device_index, workgroups_per_utterance,
                 what='set_dhtv_team')
    _settings(device_index)['dhtv_team'] = int(workgroups_per_utterance)


def dhtv_team(device_index=None):
    """The team setting in force on this thread's handle: its last set_dhtv_team, else
    PBBSS_DHTV_TEAM (read by the library when the handle is created), else 0 = automatic."""
    settings = _settings(device_index)
    if 'dhtv_team' in settings:
        return settings['dhtv_team']
    try:
        return int(os.environ.get('PBBSS_DHTV_TEAM', '0'))
    except ValueError:
        return 0


def set_dhtv_probe(enable, device_index=None):
    """pbbss_set_dhtv_probe: evaluate all plan segments at once in front of the DHTV plan and
    skip the plan when the masks are aligned already (same results; for callers that align
    every EM iteration).  `enable` True / False, or the flag word of the C call (2: the aligned
    features are not written, 3: probe + no features)."""
    flags = int(enable) if isinstance(enable, int) and not isinstance(enable, bool) else int(bool(enable))
    _lib.control('pbbss_set_dhtv_probe', device_index, flags, what='set_dhtv_probe')
    _settings(device_index)['dhtv_probe'] = flags


def dhtv_probe(device_index=None):
    """The probe flag word in force on this thread's handle (its last set_dhtv_probe, else 0)."""
    return _settings(device_index).get('dhtv_probe', 0)


# ---- N2/N3: real-embedding mixtures and joint spatial+spectral models ---------
def _real_embedding(y):
    """float32 stays float32 on the device (the kernels widen to float64 on load)."""
    t = _t()
    if y.dtype not in (t.float32, t.float64):
        y = y.to(t.float64)
    return y.contiguous()


JOINT_MAX_CLASSES = 19  # kGenMaxK (csrc/generic.hip): spatial half of pbbss_joint_fit
EMBED_MAX_CLASSES = 64  # kEmbedWideMaxK (csrc/embed_wide.hpp); K <= 8 runs on csrc/embed.hip


def _embed_check(rc, what, K):
    if rc == _lib.ERR_UNSUPPORTED and K > EMBED_MAX_CLASSES:
        raise NotImplementedError(
            f'{what}: {K} classes -- the embedding kernels serve 1 <= K <= {EMBED_MAX_CLASSES} '
            'classes and 1 <= E <= 256 features')
    _lib.check(rc, what)


def embed_log_pdf(y, kind, mean, scale):
    """pbbss_embed_log_pdf.  y (B,N,E) real; mean (B,K,E); scale (B,K) -> (B,K,N) f64."""
    t = _t()
    y = _real_embedding(y)
    B, N, E = y.shape
    K = mean.shape[1]
    out = t.empty((B, K, N), dtype=t.float64, device=y.device)
    what = f'embed_log_pdf(B={B},N={N},E={E},K={K})'
    rc = _lib.launch('pbbss_embed_log_pdf', y.device, y, y.dtype == t.float64, B, N, E, K, kind,
                     mean, scale, out, what=what, accept=_NOT_SERVED)
    _embed_check(rc, what, K)
    return out


def embed_fit(y, kind, weights, *, normalize=False, min_concentration=1e-10,
              max_concentration=500.):
    """pbbss_embed_fit.  y (B,N,E) real; weights (B,K,N) f64 -> mean (B,K,E), scale (B,K)
    ((B,K,E) per-dimension variances for EMBED_GAUSS_DIAG)."""
    t = _t()
    y = _real_embedding(y)
    B, N, E = y.shape
    K = weights.shape[1]
    assert weights.shape == (B, K, N) and weights.dtype == t.float64
    mean = t.empty((B, K, E), dtype=t.float64, device=y.device)
    scale = t.empty((B, K, E) if kind == _lib.EMBED_GAUSS_DIAG else (B, K), dtype=t.float64,
                    device=y.device)
    what = f'embed_fit(B={B},N={N},E={E},K={K})'
    rc = _lib.launch('pbbss_embed_fit', y.device, y, y.dtype == t.float64, B, N, E, K, kind,
                     bool(normalize), weights, min_concentration, max_concentration, mean, scale,
                     what=what, accept=_NOT_SERVED)
    _embed_check(rc, what, K)
    return mean, scale


def vmfmm_fit(y, K, *, gamma0=None, model=None, iterations=100, saliency=None, weight_mode=0,
              min_concentration=1e-10, max_concentration=500., final_predict=False,
              want_log_pdf=False):
    """pbbss_vmfmm_fit.  y (B,N,E) real; gamma0 (B,K,N) f64 or (iterations=0)
    model=(mean (B,K,E), concentration (B,K), weight (B,K))."""
    t = _t()
    y = _real_embedding(y)
    dev = y.device
    B, N, E = y.shape
    f64 = t.float64
    opts = _lib.MixOpts(iterations=int(iterations), kind=_lib.EMBED_VMF,
                        weight_mode=int(weight_mode), embedding_is_f64=int(y.dtype == f64),
                        final_predict=int(bool(final_predict or want_log_pdf)),
                        min_concentration=float(min_concentration),
                        max_concentration=float(max_concentration))
    mean = t.empty((B, K, E), dtype=f64, device=dev)
    conc = t.empty((B, K), dtype=f64, device=dev)
    weight = t.empty((B, K), dtype=f64, device=dev)
    aff = t.empty((B, K, N), dtype=f64, device=dev) if final_predict else None
    lp = t.empty((B, K, N), dtype=f64, device=dev) if want_log_pdf else None
    in_mean = in_conc = in_w = None
    if model is not None:
        in_mean, in_conc, in_w = model
        assert in_mean.shape == (B, K, E) and in_conc.shape == (B, K) and in_w.shape == (B, K)
    else:
        assert gamma0.shape == (B, K, N) and gamma0.dtype == f64
    what = f'vmfmm_fit(B={B},N={N},E={E},K={K})'
    rc = _lib.launch('pbbss_vmfmm_fit', dev, y, B, N, E, K, gamma0, in_mean, in_conc, in_w,
                     saliency, opts, mean, conc, weight, aff, lp, what=what, accept=_NOT_SERVED)
    _embed_check(rc, what, K)
    return dict(mean=mean, concentration=conc, weight=weight, affiliation=aff, log_pdf=lp)


def gauss_full_fit(y, weights):
    """pbbss_gauss_full_fit.  y (B,N,E) real; weights (B,K,N) f64 -> (mean (B,K,E), cov (B,K,E,E))."""
    t = _t()
    y = _real_embedding(y)
    B, N, E = y.shape
    K = weights.shape[1]
    assert weights.shape == (B, K, N) and weights.dtype == t.float64, (weights.shape, y.shape)
    mean = t.empty((B, K, E), dtype=t.float64, device=y.device)
    cov = t.empty((B, K, E, E), dtype=t.float64, device=y.device)
    _lib.launch('pbbss_gauss_full_fit', y.device, y, y.dtype == t.float64, B, N, E, K, weights,
                mean, cov, what=f'gauss_full_fit(B={B},N={N},E={E},K={K})')
    return mean, cov


def gauss_full_log_pdf(y, mean, cov):
    """pbbss_gauss_full_log_pdf.  y (B,N,E); mean (B,K,E); cov (B,K,E,E) -> ((B,K,N), status)."""
    t = _t()
    y = _real_embedding(y)
    B, N, E = y.shape
    K = mean.shape[1]
    assert mean.shape == (B, K, E) and cov.shape == (B, K, E, E), (mean.shape, cov.shape)
    out = t.empty((B, K, N), dtype=t.float64, device=y.device)
    st = t.zeros((1,), dtype=t.int32, device=y.device)
    _lib.launch('pbbss_gauss_full_log_pdf', y.device, y, y.dtype == t.float64, B, N, E, K, mean,
                cov, out, st, what=f'gauss_full_log_pdf(B={B},N={N},E={E},K={K})')
    return out, st


# ---- complex circular-symmetric Gaussian: the shape plan of csrc/ccsg.hpp ----------------------
CCSG_MAX_D = 34
CCSG_SWEEP_D = (4, 8, 16, 34)   # log-pdf instantiations: the smallest bound that holds D
CCSG_MAX_CLASS_TILE = 8         # classes in LDS at a time (fewer where D * D is large)
CCSG_LDS = 160 * 1024


def ccsg_frames(D):
    """Frames per workgroup: a frame tile of the log-pdf, a span of the fit (longer rows are split
    over workgroups)."""
    return 256 if D <= 8 else 128


def ccsg_class_tile(D):
    """Classes whose Cholesky factors the log-pdf kernel holds in LDS beside its frame tile."""
    frames = ccsg_frames(D) * (D | 1) * 16
    per_class = D * D * 16 + D * 8 + 16
    return min(CCSG_MAX_CLASS_TILE, (CCSG_LDS - frames) // per_class)


def _ccsg_frames_arg(y):
    t = _t()
    assert y.ndim == 3 and y.dtype in (t.complex64, t.complex128), (y.shape, y.dtype)
    return y.shape


def ccsg_fit(y, saliency=None, floor=None):
    """pbbss_ccsg_fit.  y (B,N,D) c64 / c128; saliency (B,K,N) f32 / f64 or None (K = 1); floor
    of the saliency sum (default: the reference's np.finfo(y.dtype).tiny) -> (B,K,D,D) c128."""
    t = _t()
    B, N, D = _ccsg_frames_arg(y)
    K = 1 if saliency is None else saliency.shape[1]
    if saliency is not None:
        assert saliency.shape == (B, K, N) and saliency.dtype in (t.float32, t.float64), (
            saliency.shape, saliency.dtype, y.shape)
    if floor is None:
        floor = np.finfo(np.complex64 if y.dtype == t.complex64 else np.complex128).tiny
    cov = t.empty((B, K, D, D), dtype=t.complex128, device=y.device)
    _lib.launch('pbbss_ccsg_fit', y.device, y, y.dtype == t.complex128, B, N, D, K, saliency,
                saliency is not None and saliency.dtype == t.float64, floor, cov,
                what=f'ccsg_fit(B={B},N={N},D={D},K={K})')
    return cov


def ccsg_log_pdf(y, covariance, want_log_det=False):
    """pbbss_ccsg_log_pdf.  y (B,N,D) c64 / c128; covariance (B,K,D,D) c128 (lower triangle and
    real diagonal are read) -> (log_pdf (B,K,N), log_det (B,K) or None, status (B,K) int32)."""
    t = _t()
    B, N, D = _ccsg_frames_arg(y)
    K = covariance.shape[1]
    assert covariance.shape == (B, K, D, D) and covariance.dtype == t.complex128, (
        covariance.shape, covariance.dtype, y.shape)
    lp = t.empty((B, K, N), dtype=t.float64, device=y.device)
    ld = t.empty((B, K), dtype=t.float64, device=y.device) if want_log_det else None
    st = t.empty((B, K), dtype=t.int32, device=y.device)
    _lib.launch('pbbss_ccsg_log_pdf', y.device, y, y.dtype == t.complex128, B, N, D, K,
                covariance, lp, ld, st, what=f'ccsg_log_pdf(B={B},N={N},D={D},K={K})')
    return lp, ld, st


# ---- WPE dereverberation: the shape plan of csrc/wpe.hpp ----------------------------------------
WPE_MAX_D = 16               # sensors
WPE_MAX_M = 96               # stacked length D * taps
WPE_TILE = 16                # edge of an FP64 MFMA tile of the correlation kernel
WPE_SPAN = 128               # frames per workgroup of the correlation kernel (ordered span sums)
WPE_CORR_TILES = (2, 4, 7)   # correlation instantiations: accumulator tiles per wavefront
WPE_APPLY_FRAMES = 256       # frames per workgroup of the filter kernel
WPE_APPLY_D = (4, 8, 16)     # filter instantiations: the smallest bound that holds D
WPE_LDS = 160 * 1024
WPE_STATISTICS = {'full': 0, 'valid': 1}


def wpe_tiles(D, taps):
    """Tiles of the lower block triangle of the extended (D * taps + D)-row Gram matrix."""
    blocks = -(-(D * taps + D) // WPE_TILE)
    return blocks * (blocks + 1) // 2


def wpe_corr_tiles_per_wave(D, taps):
    """Accumulator tiles a wavefront of the correlation kernel holds (four share the triangle)."""
    return -(-wpe_tiles(D, taps) // 4)


def wpe_solve_lds(D, taps):
    """LDS of the solver: packed lower triangle of R, the D columns of P, reciprocal diagonal."""
    M = D * taps
    return (M * (M + 1) // 2 + M * D) * 16 + M * 8


def _wpe_frames(y):
    """y: a (B, D, T) view (any strides) of c64 / c128 frames -> (view the kernels can read,
    the leading arguments of the exports)."""
    t = _t()
    assert y.ndim == 3 and y.dtype in (t.complex64, t.complex128), (tuple(y.shape), y.dtype)
    assert y.is_cuda and y.shape[0] >= 1 and y.shape[1] >= 1 and y.shape[2] >= 1, tuple(y.shape)
    if not (y.is_contiguous() or y.transpose(1, 2).is_contiguous()):
        y = y.contiguous()
    B, D, T = y.shape
    sb, sd, st = y.stride()
    return y, (_lib.view_ptr(y), y.dtype == t.complex128, B, D, T, sb, sd, st)


def _wpe_served(D, taps, delay):
    if D > WPE_MAX_D:
        raise NotImplementedError(f'wpe: D = {D} sensors, served up to WPE_MAX_D = {WPE_MAX_D}')
    if taps >= 1 and D * taps > WPE_MAX_M:
        raise NotImplementedError(
            f'wpe: D * taps = {D * taps}, served up to WPE_MAX_M = {WPE_MAX_M}')
    assert taps >= 1 and delay >= 0, (taps, delay)


def _wpe_context(psd_context):
    if psd_context == float('inf'):
        return -1
    assert psd_context >= 0 and int(psd_context) == psd_context, psd_context
    return int(psd_context)


def _wpe_like(y):
    """An uninitialised tensor with the shape and the strides of y."""
    return _t().empty_strided(tuple(y.shape), tuple(y.stride()), dtype=y.dtype, device=y.device)


def wpe(y, taps, delay, iterations, psd_context=0, statistics_mode='full'):
    """pbbss_wpe.  y: (B, D, T) view -> (x with the strides and dtype of y, status (B,) int32)."""
    y, head = _wpe_frames(y)
    B, D = y.shape[:2]
    _wpe_served(D, taps, delay)
    assert iterations >= 1, iterations
    x = _wpe_like(y)
    st = _t().empty((B,), dtype=_t().int32, device=y.device)
    _lib.launch('pbbss_wpe', y.device, *head, taps, delay, iterations, _wpe_context(psd_context),
                WPE_STATISTICS[statistics_mode], _lib.view_ptr(x), st,
                what=f'wpe(B={B},D={D},T={y.shape[2]},taps={taps},delay={delay})')
    return x, st


def wpe_power(y, psd_context=0, inverse=True):
    """pbbss_wpe_power_inverse.  y: (B, D, T) view -> (power (B, T), inverse power or None)."""
    t = _t()
    y, head = _wpe_frames(y)
    if y.shape[1] > WPE_MAX_D:
        _wpe_served(y.shape[1], 1, 0)
    B, _, T = y.shape
    power = t.empty((B, T), dtype=t.float64, device=y.device)
    inv = t.empty((B, T), dtype=t.float64, device=y.device) if inverse else None
    _lib.launch('pbbss_wpe_power_inverse', y.device, *head, _wpe_context(psd_context), power, inv,
                what=f'wpe_power(B={B},D={y.shape[1]},T={T})')
    return power, inv


def wpe_correlations(y, inverse_power, taps, delay, statistics_mode='full'):
    """pbbss_wpe_correlations.  y: (B, D, T) view; inverse_power (B, T) f64 ->
    (R (B, M, M), P (B, M, D)) c128, M = D * taps."""
    t = _t()
    y, head = _wpe_frames(y)
    B, D, T = y.shape
    _wpe_served(D, taps, delay)
    assert inverse_power.shape == (B, T) and inverse_power.dtype == t.float64, (
        tuple(inverse_power.shape), inverse_power.dtype, tuple(y.shape))
    M = D * taps
    R = t.empty((B, M, M), dtype=t.complex128, device=y.device)
    P = t.empty((B, M, D), dtype=t.complex128, device=y.device)
    _lib.launch('pbbss_wpe_correlations', y.device, *head, inverse_power.contiguous(), taps, delay,
                WPE_STATISTICS[statistics_mode], R, P,
                what=f'wpe_correlations(B={B},D={D},T={T},taps={taps},delay={delay})')
    return R, P


def wpe_filter_matrix(R, P):
    """pbbss_wpe_filter_matrix.  R (B, M, M), P (B, M, D) c128 -> (G (B, M, D), status (B,))."""
    t = _t()
    B, M, D = P.shape
    assert R.shape == (B, M, M) and R.dtype == P.dtype == t.complex128 and M % D == 0, (
        tuple(R.shape), tuple(P.shape), R.dtype, P.dtype)
    _wpe_served(D, M // D, 0)
    G = t.empty((B, M, D), dtype=t.complex128, device=P.device)
    st = t.empty((B,), dtype=t.int32, device=P.device)
    _lib.launch('pbbss_wpe_filter_matrix', P.device, R.contiguous(), P.contiguous(), B, D, M // D,
                G, st, what=f'wpe_filter_matrix(B={B},M={M},D={D})')
    return G, st


def wpe_apply_filter(y, G, taps, delay):
    """pbbss_wpe_apply_filter.  y: (B, D, T) view; G (B, D * taps, D) c128 -> x like y."""
    t = _t()
    y, head = _wpe_frames(y)
    B, D, T = y.shape
    _wpe_served(D, taps, delay)
    assert G.shape == (B, D * taps, D) and G.dtype == t.complex128, (tuple(G.shape), G.dtype)
    x = _wpe_like(y)
    _lib.launch('pbbss_wpe_apply_filter', y.device, *head, G.contiguous(), taps, delay,
                _lib.view_ptr(x), what=f'wpe_apply_filter(B={B},D={D},T={T},taps={taps})')
    return x


# the frame-recursive form: the shape plan of csrc/wpe_online.hpp
WPE_ONLINE_TILE = 32         # frames staged, and output frames written, at a time
WPE_ONLINE_MAX_RING = 2048   # D * (taps + delay): the frames kept behind the stream


def wpe_online_lds(D, taps, delay):
    """LDS of the recursive kernel: packed triangle of P, G, the frames behind the stream and a
    tile of them, a tile of output, n and x, a tile of lambda."""
    M = D * taps
    return (M * (M + 1) // 2 + M * D + (taps + delay + 2 * WPE_ONLINE_TILE) * D + M
            + WPE_MAX_D) * 16 + WPE_ONLINE_TILE * 8


def wpe_online_served(D, taps, delay):
    _wpe_served(D, taps, delay)
    if D * (taps + delay) > WPE_ONLINE_MAX_RING:
        raise NotImplementedError(f'recursive wpe: D * (taps + delay) = {D * (taps + delay)}, '
                                  f'served up to WPE_ONLINE_MAX_RING = {WPE_ONLINE_MAX_RING}')


def wpe_online(y, taps, delay, alpha, power_estimate, inv_cov, filter_taps, history, frames_seen):
    """pbbss_wpe_online.  y: (B, D, T) view; power_estimate (B, T) f64 or None; the state --
    inv_cov (B, M, M), filter_taps (B, M, D), history (B, D, taps + delay) c128, frames_seen (B,)
    int64 -- is updated in place -> (x with the strides and dtype of y, status (B,) int32)."""
    t = _t()
    y, head = _wpe_frames(y)
    B, D, T = y.shape
    wpe_online_served(D, taps, delay)
    assert 0.0 < alpha <= 1.0, alpha
    M, H = D * taps, taps + delay
    assert inv_cov.shape == (B, M, M) and filter_taps.shape == (B, M, D) and \
        history.shape == (B, D, H) and frames_seen.shape == (B,), (
            tuple(inv_cov.shape), tuple(filter_taps.shape), tuple(history.shape),
            tuple(frames_seen.shape), tuple(y.shape))
    assert inv_cov.dtype == filter_taps.dtype == history.dtype == t.complex128 and \
        frames_seen.dtype == t.int64, (inv_cov.dtype, filter_taps.dtype, history.dtype,
                                       frames_seen.dtype)
    if power_estimate is not None:
        assert power_estimate.shape == (B, T) and power_estimate.dtype == t.float64, (
            tuple(power_estimate.shape), power_estimate.dtype, tuple(y.shape))
        power_estimate = power_estimate.contiguous()
    x = _wpe_like(y)
    st = t.empty((B,), dtype=t.int32, device=y.device)
    _lib.launch('pbbss_wpe_online', y.device, *head, taps, delay, alpha, power_estimate, inv_cov,
                filter_taps, history, frames_seen, _lib.view_ptr(x), st,
                what=f'wpe_online(B={B},D={D},T={T},taps={taps},delay={delay})')
    return x, st


# the frame-recursive MVDR beamformer: the shape plan of csrc/online_bf.hpp
ONLINE_BF_MAX_D = 16   # sensors
ONLINE_BF_TILE = 32    # frames staged, and output frames written, at a time


def online_bf_served(D):
    if D > ONLINE_BF_MAX_D:
        raise NotImplementedError(f'recursive mvdr: D = {D} sensors, served up to '
                                  f'ONLINE_BF_MAX_D = {ONLINE_BF_MAX_D}')


def online_mvdr(y, target_mask, noise_mask, alpha, ref_channel, target_psd, noise_inv,
                frames_seen, want_vector=False):
    """pbbss_online_mvdr.  y: (B, D, T) view; the masks (B, T) f32 / f64 of one dtype; the state
    -- target_psd, noise_inv (B, D, D) c128, frames_seen (B,) int64 -- is updated in place ->
    (x (B, T) of the dtype of y, w (T, B, D) c128 or None, status (B,) int32)."""
    t = _t()
    y, head = _wpe_frames(y)
    B, D, T = y.shape
    online_bf_served(D)
    assert 0.0 < alpha <= 1.0, alpha
    assert 0 <= ref_channel < D, (ref_channel, D)
    assert target_mask.shape == noise_mask.shape == (B, T) and \
        target_mask.dtype == noise_mask.dtype and target_mask.dtype in (t.float32, t.float64), (
            tuple(target_mask.shape), tuple(noise_mask.shape), target_mask.dtype, noise_mask.dtype,
            tuple(y.shape))
    assert target_psd.shape == noise_inv.shape == (B, D, D) and frames_seen.shape == (B,), (
        tuple(target_psd.shape), tuple(noise_inv.shape), tuple(frames_seen.shape), tuple(y.shape))
    assert target_psd.dtype == noise_inv.dtype == t.complex128 and frames_seen.dtype == t.int64, (
        target_psd.dtype, noise_inv.dtype, frames_seen.dtype)
    x = t.empty((B, T), dtype=y.dtype, device=y.device)
    w = t.empty((T, B, D), dtype=t.complex128, device=y.device) if want_vector else None
    st = t.empty((B,), dtype=t.int32, device=y.device)
    _lib.launch('pbbss_online_mvdr', y.device, *head, target_mask.contiguous(),
                noise_mask.contiguous(), target_mask.dtype == t.float64, alpha, ref_channel,
                target_psd, noise_inv, frames_seen, x, w, st,
                what=f'online_mvdr(B={B},D={D},T={T})')
    return x, w, st


# the frame-recursive cACGMM mask estimator: the shape plan of csrc/online_cacgmm.hpp
ONLINE_CACGMM_MAX_D = 16   # sensors
ONLINE_CACGMM_MAX_K = 8    # classes
ONLINE_CACGMM_TILE = 32    # frames staged, and output frames written, at a time


def online_cacgmm_served(D, K):
    if D < 2 or K < 2:
        raise ValueError(f'recursive cacgmm needs D >= 2 sensors and K >= 2 classes, got D = {D}, '
                         f'K = {K}')
    if D > ONLINE_CACGMM_MAX_D:
        raise NotImplementedError(f'recursive cacgmm: D = {D} sensors, served up to '
                                  f'ONLINE_CACGMM_MAX_D = {ONLINE_CACGMM_MAX_D}')
    if K > ONLINE_CACGMM_MAX_K:
        raise NotImplementedError(f'recursive cacgmm: K = {K} classes, served up to '
                                  f'ONLINE_CACGMM_MAX_K = {ONLINE_CACGMM_MAX_K}')


def online_cacgmm(y, alpha, affiliation_eps, update_weight, precision, log_determinant, count,
                  weight, frames_seen, want_q=False):
    """pbbss_online_cacgmm.  y: (B, D, T) view; the state -- precision (B, K, D, D) c128,
    log_determinant, count, weight (B, K) f64, frames_seen (B,) int64 -- is updated in place ->
    (affiliation (B, K, T) f64, quadratic_form (B, K, T) f64 or None, status (B,) int32)."""
    t = _t()
    y, head = _wpe_frames(y)
    B, D, T = y.shape
    K = precision.shape[1] if precision.ndim == 4 else 0
    online_cacgmm_served(D, K)
    assert 0.0 < alpha <= 1.0, alpha
    assert 0.0 <= affiliation_eps < 0.5, affiliation_eps
    assert precision.shape == (B, K, D, D) and frames_seen.shape == (B,) and \
        log_determinant.shape == count.shape == weight.shape == (B, K), (
            tuple(precision.shape), tuple(log_determinant.shape), tuple(count.shape),
            tuple(weight.shape), tuple(frames_seen.shape), tuple(y.shape))
    assert precision.dtype == t.complex128 and frames_seen.dtype == t.int64 and \
        log_determinant.dtype == count.dtype == weight.dtype == t.float64, (
            precision.dtype, log_determinant.dtype, count.dtype, weight.dtype, frames_seen.dtype)
    aff = t.empty((B, K, T), dtype=t.float64, device=y.device)
    q = t.empty((B, K, T), dtype=t.float64, device=y.device) if want_q else None
    st = t.empty((B,), dtype=t.int32, device=y.device)
    _lib.launch('pbbss_online_cacgmm', y.device, head[0], head[1], B, D, K, *head[4:], alpha,
                affiliation_eps, bool(update_weight), precision, log_determinant, count, weight,
                frames_seen, aff, q, st, what=f'online_cacgmm(B={B},D={D},K={K},T={T})')
    return aff, q, st


def gmm_fit(y, K, *, gamma0=None, model=None, iterations=100, saliency=None, weight_mode=0,
            fixed_covariance=None, final_predict=False, want_log_pdf=False):
    """pbbss_gmm_fit (spherical covariances).  y (B,N,E) real, used as given (no row
    normalisation); gamma0 (B,K,N) f64 or (iterations=0) model=(mean (B,K,E),
    covariance (B,K), weight (B,K)); fixed_covariance (B,K) or None."""
    t = _t()
    y = _real_embedding(y)
    dev = y.device
    B, N, E = y.shape
    f64 = t.float64
    opts = _lib.MixOpts(iterations=int(iterations), kind=_lib.EMBED_GAUSS_SPHERICAL,
                        weight_mode=int(weight_mode), embedding_is_f64=int(y.dtype == f64),
                        final_predict=int(bool(final_predict or want_log_pdf)))
    mean = t.empty((B, K, E), dtype=f64, device=dev)
    cov = t.empty((B, K), dtype=f64, device=dev)
    weight = t.empty((B, K), dtype=f64, device=dev)
    aff = t.empty((B, K, N), dtype=f64, device=dev) if final_predict else None
    lp = t.empty((B, K, N), dtype=f64, device=dev) if want_log_pdf else None
    in_mean = in_cov = in_w = None
    if model is not None:
        in_mean, in_cov, in_w = model
        assert in_mean.shape == (B, K, E) and in_cov.shape == (B, K) and in_w.shape == (B, K)
    else:
        assert gamma0.shape == (B, K, N) and gamma0.dtype == f64
    if fixed_covariance is not None:
        assert fixed_covariance.shape == (B, K) and fixed_covariance.dtype == f64
    what = f'gmm_fit(B={B},N={N},E={E},K={K})'
    rc = _lib.launch('pbbss_gmm_fit', dev, y, B, N, E, K, gamma0, in_mean, in_cov, in_w, saliency,
                     fixed_covariance, opts, mean, cov, weight, aff, lp, what=what,
                     accept=_NOT_SERVED)
    _embed_check(rc, what, K)
    return dict(mean=mean, covariance=cov, weight=weight, affiliation=aff, log_pdf=lp)


def gmm_full_fit(y, K, *, gamma0=None, model=None, iterations=100, saliency=None, weight_mode=0,
                 fixed_covariance=None, final_predict=False, want_log_pdf=False):
    """pbbss_gmm_full_fit (full covariances, E <= 63).  As gmm_fit with covariance (B,K,E,E).
    Returns the status word too (non-zero: a covariance was not positive definite)."""
    t = _t()
    y = _real_embedding(y)
    dev = y.device
    B, N, E = y.shape
    f64 = t.float64
    opts = _lib.MixOpts(iterations=int(iterations), kind=_lib.EMBED_GAUSS_SPHERICAL,
                        weight_mode=int(weight_mode), embedding_is_f64=int(y.dtype == f64),
                        final_predict=int(bool(final_predict or want_log_pdf)))
    mean = t.empty((B, K, E), dtype=f64, device=dev)
    cov = t.empty((B, K, E, E), dtype=f64, device=dev)
    weight = t.empty((B, K), dtype=f64, device=dev)
    aff = t.empty((B, K, N), dtype=f64, device=dev) if final_predict else None
    lp = t.empty((B, K, N), dtype=f64, device=dev) if want_log_pdf else None
    st = t.zeros((1,), dtype=t.int32, device=dev)
    in_mean = in_cov = in_w = None
    if model is not None:
        in_mean, in_cov, in_w = model
        assert in_mean.shape == (B, K, E) and in_cov.shape == (B, K, E, E) and in_w.shape == (B, K)
    else:
        assert gamma0.shape == (B, K, N) and gamma0.dtype == f64
    if fixed_covariance is not None:
        assert fixed_covariance.shape == (B, K, E, E) and fixed_covariance.dtype == f64
    _lib.launch('pbbss_gmm_full_fit', dev, y, B, N, E, K, gamma0, in_mean, in_cov, in_w, saliency,
                fixed_covariance, opts, mean, cov, weight, aff, lp, st,
                what=f'gmm_full_fit(B={B},N={N},E={E},K={K})')
    return dict(mean=mean, covariance=cov, weight=weight, affiliation=aff, log_pdf=lp, status=st)


def estimate_mixture_weight(affiliation, saliency, reduce_inner, reduce_n):
    """pbbss_estimate_mixture_weight: affiliation (Bo, Bi, K, N) f64, saliency (Bo, Bi, N) or
    None -> (Bo, 1 if reduce_inner else Bi, K, 1 if reduce_n else N); None where the kernel does
    not serve the shape (a saliency with more than 16 classes): the caller takes the host formula."""
    t = _t()
    Bo, Bi, K, N = affiliation.shape
    out = t.empty((Bo, 1 if reduce_inner else Bi, K, 1 if reduce_n else N), dtype=t.float64,
                  device=affiliation.device)
    rc = _lib.launch('pbbss_estimate_mixture_weight', affiliation.device, affiliation, saliency,
                     Bo, Bi, K, N, bool(reduce_inner), bool(reduce_n), out,
                     what=f'estimate_mixture_weight(Bo={Bo},Bi={Bi},K={K},N={N})',
                     accept=_NOT_SERVED)
    return None if rc == _lib.ERR_UNSUPPORTED else out


def log_pdf_to_affiliation(log_pdf, weight, activity=None, affiliation_eps=0.):
    """pbbss_log_pdf_to_affiliation: log_pdf (B,K,N) f64; weight a tensor that broadcasts against
    it -- (B,K,1), (K,1), (1,K,N), (B,1,N) ...: singleton axes become zero strides -> (B,K,N)."""
    t = _t()
    B, K, N = log_pdf.shape
    w, st = _broadcast_weight(weight, (B, K, N))
    out = t.empty((B, K, N), dtype=t.float64, device=log_pdf.device)
    if activity is not None:
        assert activity.shape == (B, K, N) and activity.dtype == t.uint8
    _lib.launch('pbbss_log_pdf_to_affiliation', log_pdf.device, log_pdf.contiguous(), B, K, N, w,
                st[0], st[1], st[2], activity, affiliation_eps, out,
                what=f'log_pdf_to_affiliation(B={B},K={K},N={N})')
    return out


def _broadcast_weight(weight, shape):
    """weight -> (contiguous float64 tensor, strides with 0 on singleton axes) against `shape`."""
    t = _t()
    w = weight.to(t.float64)
    while w.ndim < len(shape):
        w = w.unsqueeze(0)
    assert w.ndim == len(shape) and all(a in (1, b) for a, b in zip(w.shape, shape)), \
        (tuple(w.shape), tuple(shape))
    w = w.contiguous()
    return w, [0 if w.shape[i] == 1 else w.stride(i) for i in range(w.ndim)]


def log_pdf_to_affiliation_inline_pa(spatial_log_pdf, spectral_log_pdf, weight, activity=None,
                                     affiliation_eps=0., want_permutation=False):
    """pbbss_log_pdf_to_affiliation_inline_pa: both log-pdfs (F,K,T) f64, weight broadcastable."""
    t = _t()
    F, K, T = spatial_log_pdf.shape
    assert spectral_log_pdf.shape == (F, K, T), (spectral_log_pdf.shape, (F, K, T))
    if K > 6:
        raise NotImplementedError(f'inline permutation alignment searches K! permutations per bin: '
                                  f'K <= 6 is served, got K={K}')
    w, st = _broadcast_weight(weight, (F, K, T))
    dev = spatial_log_pdf.device
    out = t.empty((F, K, T), dtype=t.float64, device=dev)
    perm = t.empty((F, K), dtype=t.int32, device=dev) if want_permutation else None
    if activity is not None:
        assert activity.shape == (F, K, T) and activity.dtype == t.uint8
    _lib.launch('pbbss_log_pdf_to_affiliation_inline_pa', dev,
                spatial_log_pdf.to(t.float64).contiguous(),
                spectral_log_pdf.to(t.float64).contiguous(), F, K, T, w, st[0], st[1], st[2],
                activity, affiliation_eps, out, perm,
                what=f'log_pdf_to_affiliation_inline_pa(F={F},K={K},T={T})')
    return (out, perm) if want_permutation else out


def joint_weight_shape(weight_mode, F, K, T):
    return {_lib.JOINT_WEIGHT_FK: (F, K), _lib.JOINT_WEIGHT_UNIFORM: (), _lib.JOINT_WEIGHT_K: (K,),
            _lib.JOINT_WEIGHT_KT: (K, T), _lib.JOINT_WEIGHT_CONST: ()}[weight_mode]


def joint_fit(observation, embedding, K, kind, *, gamma0=None, model=None, iterations=100,
              saliency=None, weight_mode=0, covariance_norm=1, eigenvalue_floor=1e-10,
              affiliation_eps=1e-10, spatial_weight=1., spectral_weight=1., inline_pa=False,
              min_concentration=1e-10, max_concentration=500., fixed_scale=None,
              final_predict=False, check_status=True, sharded=False):
    """pbbss_joint_fit.  observation (F,T,D) complex, embedding (F,T,E) real;
    gamma0 (F,K,T) f64 or (iterations=0) model=(eigvec, eigval, weight, mean (K,E), scale);
    scale: (K,) concentration / spherical variance, (K,E) diagonal variances, (K,E,E) full
    covariance, by `kind`."""
    t = _t()
    embedding = _real_embedding(embedding)
    dev = observation.device
    F, T, D = observation.shape
    E = embedding.shape[-1]
    assert embedding.shape == (F, T, E)
    f64 = t.float64
    opts = _lib.MixOpts(iterations=int(iterations), kind=int(kind), weight_mode=int(weight_mode),
                        embedding_is_f64=int(embedding.dtype == f64),
                        obs_is_c128=int(observation.dtype == t.complex128),
                        final_predict=int(bool(final_predict)), inline_pa=int(bool(inline_pa)),
                        covariance_norm=int(covariance_norm),
                        min_concentration=float(min_concentration),
                        max_concentration=float(max_concentration),
                        affiliation_eps=float(affiliation_eps),
                        eigenvalue_floor=float(eigenvalue_floor),
                        spatial_weight=float(spatial_weight),
                        spectral_weight=float(spectral_weight), sharded=int(bool(sharded)))
    wshape = joint_weight_shape(weight_mode, F, K, T)
    eigvec = t.empty((F, K, D, D), dtype=t.complex128, device=dev)
    eigval = t.empty((F, K, D), dtype=f64, device=dev)
    weight = t.empty(wshape, dtype=f64, device=dev)
    mean = t.empty((K, E), dtype=f64, device=dev)
    scale_shape = {_lib.EMBED_GAUSS_FULL: (K, E, E), _lib.EMBED_GAUSS_DIAG: (K, E)}.get(kind, (K,))
    scale = t.empty(scale_shape, dtype=f64, device=dev)
    status = t.zeros((F, K), dtype=t.int32, device=dev)
    aff = t.empty((F, K, T), dtype=f64, device=dev) if final_predict else None
    in_vec = in_val = in_w = in_mean = None
    in_scale = fixed_scale
    if model is not None:
        in_vec, in_val, in_w, in_mean, in_scale = model
        assert in_vec.shape == (F, K, D, D) and in_val.shape == (F, K, D)
        assert tuple(in_w.shape) == tuple(wshape) and in_mean.shape == (K, E)
        assert tuple(in_scale.shape) == scale_shape, (tuple(in_scale.shape), scale_shape)
    else:
        assert gamma0.shape == (F, K, T) and gamma0.dtype == f64
    what = f'joint_fit(F={F},T={T},D={D},E={E},K={K})'
    rc = _lib.launch('pbbss_joint_fit', dev, observation, embedding, F, T, D, E, K, gamma0, in_vec,
                     in_val, in_w, in_mean, in_scale, saliency, opts, eigvec, eigval, weight, mean,
                     scale, status, aff, what=what, accept=_NOT_SERVED)
    if rc == _lib.ERR_UNSUPPORTED and (K > JOINT_MAX_CLASSES or (inline_pa and K > 6)
                                       or (sharded and K > 8)):
        raise NotImplementedError(
            f'{what}: the joint models serve 1 <= K <= '
            f'{JOINT_MAX_CLASSES} classes (the generic-size spatial kernels), inline permutation '
            'alignment 1 <= K <= 6, bin-sharded fits 1 <= K <= 8')
    _lib.check(rc, what)
    if kind == _lib.EMBED_GAUSS_FULL and int(status[0, 0].item()) & _lib.ST_NOT_POSDEF:
        raise ValueError(  # sklearn's _compute_precision_cholesky via gaussian.py:26
            'Fitting the mixture model failed because some components have ill-defined empirical '
            'covariance (not positive definite)')
    if check_status and iterations > 0:
        _status_raise_em(status, 'joint model fit')
    return dict(eigvec=eigvec, eigval=eigval, weight=weight, mean=mean, scale=scale,
                status=status, affiliation=aff)


# ---- N4: remaining beamformer family ------------------------------------------
def lcmv(atf, response, noise):
    """pbbss_lcmv.  atf (K,F,D), response (K), noise (F,D,D) c128 -> w (F,D), status (F)."""
    t = _t()
    K, F, D = atf.shape
    w = t.empty((F, D), dtype=t.complex128, device=atf.device)
    st = t.zeros((F,), dtype=t.int32, device=atf.device)
    _lib.launch('pbbss_lcmv', atf.device, atf, response, noise, F, D, K, w, st,
                what=f'lcmv(K={K},F={F},D={D})')
    return w, st


def phase_correction(vector):
    """pbbss_phase_correction.  vector (..., F, D) c128 contiguous."""
    t = _t()
    F, D = vector.shape[-2:]
    two_d = vector.ndim == 2
    lead = 1 if two_d else vector.shape[0]
    rest = 1 if two_d else int(np.prod(vector.shape[1:-2], dtype=np.int64))
    out = t.empty_like(vector)
    scratch = t.empty((max(lead * rest * (F - 1), 1),), dtype=t.complex128, device=vector.device)
    _lib.launch('pbbss_phase_correction', vector.device, vector, lead, rest, F, D, two_d, scratch,
                out, what=f'phase_correction(shape={tuple(vector.shape)})')
    return out


def snr_postfilter(w, target, noise):
    t = _t()
    F, D = w.shape
    out = t.empty((F,), dtype=t.complex128, device=w.device)
    _lib.launch('pbbss_snr_postfilter', w.device, w, target, noise, F, D, out,
                what=f'snr_postfilter(F={F},D={D})')
    return out


def reference_channel_terms(w_mat, target, noise):
    """pbbss_reference_channel_terms.  (F,D,D) c128 x 3 -> num, den (F,D) c128."""
    t = _t()
    F, D, _ = w_mat.shape
    num = t.empty((F, D), dtype=t.complex128, device=w_mat.device)
    den = t.empty((F, D), dtype=t.complex128, device=w_mat.device)
    _lib.launch('pbbss_reference_channel_terms', w_mat.device, w_mat, target, noise, F, D, num,
                den, what=f'reference_channel_terms(F={F},D={D})')
    return num, den


def rank_one_approximation(covariance, vector):
    """pbbss_rank_one_approximation.  (N,D,D), (N,D) c128 -> (N,D,D)."""
    t = _t()
    N, D = vector.shape
    out = t.empty((N, D, D), dtype=t.complex128, device=vector.device)
    _lib.launch('pbbss_rank_one_approximation', vector.device, covariance, vector, N, D, out,
                what=f'rank_one_approximation(N={N},D={D})')
    return out


def matvec(matrix, vector):
    """pbbss_matvec.  (N,D,D), (N,D) c128 -> (N,D)."""
    t = _t()
    N, D = vector.shape
    out = t.empty((N, D), dtype=t.complex128, device=vector.device)
    _lib.launch('pbbss_matvec', vector.device, matrix, vector, N, D, out,
                what=f'matvec(N={N},D={D})')
    return out


def distortionless_normalization(w, atf, noise):
    t = _t()
    F, D = w.shape
    out = t.empty((F, D), dtype=t.complex128, device=w.device)
    _lib.launch('pbbss_distortionless_normalization', w.device, w, atf, noise, F, D, out,
                what=f'distortionless_normalization(F={F},D={D})')
    return out


def zero_degree_normalization(vector, reference_channel):
    t = _t()
    N, D = vector.shape
    out = t.empty_like(vector)
    _lib.launch('pbbss_zero_degree_normalization', vector.device, vector, N, D,
                int(reference_channel) % D, out, what=f'zero_degree_normalization(N={N},D={D})')
    return out


def condition_covariance(x, gamma):
    t = _t()
    N, D, _ = x.shape
    out = t.empty_like(x)
    _lib.launch('pbbss_condition_covariance', x.device, x, N, D, gamma, out,
                what=f'condition_covariance(N={N},D={D})')
    return out


def apply_online_bf(vector, mix):
    """pbbss_apply_online_beamforming_vector.  vector (T,F,D) c128, mix (F,D,T) c64/c128."""
    t = _t()
    T, F, D = vector.shape
    out = t.empty((F, T), dtype=t.complex128, device=mix.device)
    _lib.launch('pbbss_apply_online_beamforming_vector', mix.device, vector, mix,
                mix.dtype == t.complex128, F, T, D, out, what=f'apply_online_bf(T={T},F={F},D={D})')
    return out


def stft_num_frames(num_samples, size, shift, window_length, fading=True, pad=True):
    """pbbss_stft_num_frames (host arithmetic only)."""
    n = _lib.load().pbbss_stft_num_frames(int(num_samples), int(size), int(shift),
                                          int(window_length), int(bool(fading)), int(bool(pad)))
    if n < 0:
        _lib.check(n, f'stft_num_frames(N={num_samples},size={size},shift={shift})')
    return n


def stft(x, size, shift, window, *, fading=True, pad=True, layout=0, out_c128=True):
    """pbbss_stft.  x (C,N) float32/float64, window (window_length) f64 on the device.

    Returns (C,T,F) [layout 0] or (F,T,C) [layout 1] complex128 / complex64, F = size//2+1."""
    t = _t()
    C, N = x.shape
    wl = int(window.shape[0])
    T = stft_num_frames(N, size, shift, wl, fading, pad)
    if T <= 0:
        raise ValueError(f'stft: no complete frame in {N} samples (size={size}, pad={pad})')
    F = size // 2 + 1
    shape = (C, T, F) if layout == 0 else (F, T, C)
    out = t.empty(shape, dtype=t.complex128 if out_c128 else t.complex64, device=x.device)
    _lib.launch('pbbss_stft', x.device, x, x.dtype == t.float64, C, N, size, shift, wl, window,
                bool(fading), bool(pad), layout, bool(out_c128), out,
                what=f'stft(C={C},N={N},size={size},shift={shift},window_length={wl})')
    return out


def istft(X, size, shift, synthesis_window, *, fading=True):
    """pbbss_istft.  X (C,T,F) complex64/complex128 -> (C, n_out) float64."""
    t = _t()
    C, T, F = X.shape
    wl = int(synthesis_window.shape[0])
    n_out = T * shift + wl - shift - (2 * (wl - shift) if fading else 0)
    if n_out <= 0:
        raise ValueError(f'istft: {T} frames give no output samples')
    out = t.empty((C, n_out), dtype=t.float64, device=X.device)
    _lib.launch('pbbss_istft', X.device, X, X.dtype == t.complex128, C, T, size, shift, wl,
                synthesis_window, bool(fading), out, n_out,
                what=f'istft(C={C},T={T},size={size},shift={shift},window_length={wl})')
    return out


def stft_stream(x, n, hist_in, hist_out, samples_seen, frames_seen, m, size, shift, window, *,
                fading=True, flush=False, layout=0, out_c128=True):
    """pbbss_stft_stream.  x (C, n) float32/float64 (None for n = 0), hist_in / hist_out (C, H)
    float64, H = max(1, window_length - 1), two different buffers; the counters are host integers.

    Writes the history behind the block into hist_out and returns the m frames as (C, m, F)
    [layout 0] or (F, m, C) [layout 1]."""
    t = _t()
    C = hist_in.shape[0]
    wl = int(window.shape[0])
    F = size // 2 + 1
    shape = (C, m, F) if layout == 0 else (F, m, C)
    out = t.empty(shape, dtype=t.complex128 if out_c128 else t.complex64, device=hist_in.device)
    _lib.launch_stream('stft', hist_in.device, x, x is not None and x.dtype == t.float64, C, n,
                       hist_in, hist_out, samples_seen, frames_seen, m, bool(flush), size, shift,
                       wl, window, bool(fading), layout, bool(out_c128), out if m else None,
                       what=f'stft_stream(C={C},n={n},m={m},size={size},shift={shift},'
                            f'window_length={wl})')
    return out


def istft_stream(X, size, shift, synthesis_window, tail, skip):
    """pbbss_istft_stream.  X (rows, m, F) complex64/complex128, any strides; tail
    (rows, window_length - shift) float64 contiguous, updated in place ->
    (rows, m * shift - skip) float64."""
    t = _t()
    rows, m, F = X.shape
    wl = int(synthesis_window.shape[0])
    n_out = max(0, m * shift - skip)
    out = t.empty((rows, n_out), dtype=t.float64, device=X.device)
    _lib.launch_stream('istft', X.device, _lib.view_ptr(X), X.dtype == t.complex128, rows, m,
                       X.stride(0), X.stride(1), X.stride(2), size, shift, wl, synthesis_window,
                       tail, skip, out if n_out else None, n_out,
                       what=f'istft_stream(rows={rows},m={m},size={size},shift={shift},'
                            f'window_length={wl})')
    return out


def griffin_lim(X, y, x_hat, size, shift, analysis_window, synthesis_window, *, fading=False,
                iterations=1):
    """pbbss_griffin_lim.  X (B,K,T,F) complex64/complex128, y (B,n) float64 (MISI) or None
    (Griffin-Lim), x_hat (B,K,n) float64: the current estimate, left untouched.

    Returns (x_hat, X_dash_dash, X_dash) after `iterations` iterations: (B,K,n) float64 and the
    last iteration's two (B,K,T,F) complex128 spectra."""
    t = _t()
    B, K, T, F = X.shape
    n = x_hat.shape[-1]
    out = x_hat.clone()
    X_dash_dash = t.empty((B, K, T, F), dtype=t.complex128, device=X.device)
    X_dash = t.empty_like(X_dash_dash)
    _lib.launch('pbbss_griffin_lim', X.device, X, X.dtype == t.complex128, y, B, K, T, size, shift,
                analysis_window, synthesis_window, bool(fading), iterations, out, X_dash_dash,
                X_dash, n,
                what=f'griffin_lim(B={B},K={K},T={T},size={size},shift={shift},'
                     f'iterations={iterations},misi={y is not None})')
    return out, X_dash_dash, X_dash
