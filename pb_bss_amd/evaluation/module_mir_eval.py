"""BSS-Eval SDR, SIR and SAR (reference: pb_bss/evaluation/module_mir_eval.py, which wraps
`mir_eval.separation.bss_eval_sources`) on the device, without the `mir_eval` package.

The metric is defined by mathematics (Vincent et al. 2006, BSS Eval 3.0): every estimate,
zero-padded by `filter_length - 1` samples, is projected by least squares onto the
`filter_length` delayed copies of one reference and onto those of all references; the three
energy ratios of the pieces are SDR, SIR and SAR.  One call into csrc/bss_eval.hip
(`pbbss_bss_eval`) does all of it for a batch: lagged correlations, a blocked Cholesky
factorisation of the block-Toeplitz normal equations, the filters applied in one streaming pass,
the search for the assignment with the largest mean SIR.  float64 throughout (float32 input is
widened in registers).

Where the factorisation refuses a matrix (status NOT_POSDEF: linearly dependent references,
periodic signals), that item's normal equations are fetched (`pbbss_bss_eval_system`), solved
with `numpy.linalg.lstsq` on the host and the energies are computed on the device from those
filters (`pbbss_bss_eval_filters`) -- the same step `mir_eval` takes on a LinAlgError.
"""
import numpy as np

from .. import _lib
from . import _signals

__all__ = ['mir_eval_sources']

SPAN = 2048  # samples one correlation workgroup owns (csrc/bss_eval.hpp: kBssCorrSpan)
SYNTHESIS_SPAN = 1024  # output samples one synthesis workgroup owns (kBssSynSpan)
MAX_FILTER_LENGTH = 512  # csrc/bss_eval.hpp: kBssMaxFilter
_MAX_SOURCES = 8  # csrc/bss_eval.hpp: kBssMaxSources


def _batched(x, N):
    """(K, *mid, N) device tensor -> (view (B, K, N) with a unit sample stride, mid)"""
    if x.stride(-1) != 1 and N != 1:
        x = x.contiguous()
    mid = tuple(x.shape[1:-1])
    K = x.shape[0]
    merged = _signals.collapse([(size, x.stride(1 + a), 0) for a, size in enumerate(mid)])
    if len(merged) > 1:
        x = x.movedim(0, -2).contiguous().movedim(-2, 0)  # (*mid, K, N) in memory
        merged = _signals.collapse([(size, x.stride(1 + a), 0) for a, size in enumerate(mid)])
    B = int(np.prod(mid, dtype=np.int64))
    batch_stride = merged[0][1] if merged else 0
    return x.as_strided((B, K, x.shape[-1]), (batch_stride, x.stride(0), 1),
                        x.storage_offset()), mid


def _common(ref, est, filter_length):
    """the arguments the three bss_eval exports share, behind the handle"""
    B, K, N = ref.shape
    return (_lib.view_ptr(ref), _lib.view_ptr(est), _signals.dtype_code(ref), B, K, est.shape[1],
            N, ref.stride(0) if B > 1 else 0, ref.stride(1), est.stride(0), est.stride(1),
            filter_length)


def _outputs(t, B, K, device):
    values = t.empty((3, B, K), dtype=t.float64, device=device)
    selection = t.empty((B, K), dtype=t.int64, device=device)
    status = t.empty((B,), dtype=t.int32, device=device)
    return values, selection, status


def _host_solve(ref, est, filter_length, compute_permutation):
    """the items of (ref, est) through the normal equations on the host: lstsq filters, then the
    energies on the device"""
    t = _lib.torch()
    B, K, N = ref.shape
    Ke, L = est.shape[1], filter_length
    n = K * L
    shared = B > 1 and ref.stride(0) == 0
    gram = t.empty((1 if shared else B, n, n), dtype=t.float64, device=ref.device)
    rhs = t.empty((B, Ke, n), dtype=t.float64, device=ref.device)
    common = _common(ref, est, L)
    _lib.launch('pbbss_bss_eval_system', ref.device, *common, gram, rhs, what='bss_eval_system')
    G, D = _lib.to_host(gram), _lib.to_host(rhs)
    blocks = [slice(j * L, (j + 1) * L) for j in range(K)]

    def filters(Gb, Db):
        """Gb (n, n), Db (R, n) -> all (R, n), single (R, K, L)"""
        f_all = np.linalg.lstsq(Gb, Db.T, rcond=None)[0].T
        f_single = np.stack([np.linalg.lstsq(Gb[blk, blk], Db[:, blk].T, rcond=None)[0].T
                             for blk in blocks], axis=1)
        return f_all, f_single

    if shared:
        f_all, f_single = filters(G[0], D.reshape(B * Ke, n))
    else:
        pairs = [filters(G[b], D[b]) for b in range(B)]
        f_all = np.stack([p[0] for p in pairs])
        f_single = np.stack([p[1] for p in pairs])
    f_all = np.ascontiguousarray(f_all.reshape(B, Ke, n))
    f_single = np.ascontiguousarray(f_single.reshape(B, Ke, K, L))
    values, selection, status = _outputs(t, B, K, ref.device)
    fa = t.from_numpy(f_all).to(ref.device)
    fs = t.from_numpy(f_single).to(ref.device)
    _lib.launch('pbbss_bss_eval_filters', ref.device, *common, compute_permutation, fa, fs,
                values[0], values[1], values[2], selection, None, status, what='bss_eval_filters')
    return values, selection


def _device_call(ref, est, filter_length, compute_permutation, info=None):
    """ref (B, K, N), est (B, Ke, N) views on one device -> values (3, B, K), selection (B, K)"""
    t = _lib.torch()
    B, K, N = ref.shape
    Ke = est.shape[1]
    values, selection, status = _outputs(t, B, K, ref.device)
    tables = t.empty((B, 3, Ke, K), dtype=t.float64, device=ref.device) if info is not None \
        else None
    _lib.launch('pbbss_bss_eval', ref.device, *_common(ref, est, filter_length),
                compute_permutation, values[0], values[1], values[2], selection, tables, status,
                what=f'mir_eval_sources(B={B}, K={K}, Ke={Ke}, N={N}, '
                     f'filter_length={filter_length})')
    st = _lib.to_host(status)
    if info is not None:
        info['status'] = st
        info['tables'] = tables
    if (st & _lib.ST_ZERO_SIGNAL).any():
        raise ValueError(
            'All the reference sources and all the estimated sources should be non-silent (not '
            'all-zeros): the BSS-Eval metrics are undefined for a silent signal.')
    refused = np.flatnonzero(st & _lib.ST_NOT_POSDEF)
    if refused.size:
        if B > 1 and ref.stride(0) == 0:  # one factorisation for all items
            values, selection = _host_solve(ref, est, filter_length, compute_permutation)
        else:
            idx = t.from_numpy(refused).to(ref.device)
            v, s = _host_solve(ref.index_select(0, idx), est.index_select(0, idx),
                               filter_length, compute_permutation)
            values[:, idx] = v
            selection[idx] = s
    return values, selection


def _evaluate(reference, estimation, compute_permutation, filter_length, _info=None):
    """argument checks and the device call -> values (3, B, K), selection (B, K), K, the axes
    between the first and the last, where the result goes.  `_info` (a dict) receives the
    'status' words and the (B, 3, Ke, K) 'tables' of the device solve."""
    like_torch, home = _signals.home_of(reference, estimation)
    if not _lib.is_torch(reference):
        reference = np.asarray(reference)
    if not _lib.is_torch(estimation):
        estimation = np.asarray(estimation)
    r_shape, e_shape = tuple(reference.shape), tuple(estimation.shape)
    if len(r_shape) < 2:
        raise ValueError(f'Strange input shape: {r_shape}')
    if len(r_shape) == 2:
        assert len(e_shape) == 2, e_shape
        assert r_shape[1] == e_shape[1], (r_shape, e_shape)
    else:
        assert r_shape[1:] == e_shape[1:], (r_shape, e_shape)
    K, Ke = r_shape[0], e_shape[0]
    if Ke == K + 1:
        if not compute_permutation:
            raise NotImplementedError(compute_permutation, 'with K + 1')
    elif Ke != K:
        raise ValueError(f'Shapes do not fit: {r_shape} vs. {e_shape}')
    if not 1 <= K <= _MAX_SOURCES or Ke > _MAX_SOURCES:
        raise NotImplementedError(
            f'{K} sources, {Ke} estimates: the BSS-Eval kernels take 1 to {_MAX_SOURCES} of each')
    filter_length = int(filter_length)
    if not 1 <= filter_length <= MAX_FILTER_LENGTH:
        raise NotImplementedError(
            f'filter_length={filter_length}: the BSS-Eval kernels take 1 to {MAX_FILTER_LENGTH}')
    N = r_shape[-1]
    if N == 0:
        raise ValueError(f'empty signal: shape {r_shape}')

    _lib.require_gpu()
    ref = _signals.device_signal(reference, complex_ok=False)
    est = _signals.device_signal(estimation, complex_ok=False)
    if est.device != ref.device:
        est = est.to(ref.device)
    ref, est = _signals.common_dtype(ref, est)
    ref_b, mid = _batched(ref, N)
    est_b, _ = _batched(est, N)
    if ref_b.shape[0] == 0:
        raise ValueError(f'empty signal: shape {r_shape}')
    values, selection = _device_call(ref_b, est_b, filter_length, compute_permutation, _info)
    return values, selection, K, mid, like_torch, home


def mir_eval_sources(
        reference,
        estimation,
        return_dict=False,
        compute_permutation=True,
        *,
        filter_length=512
):
    """BSS-Eval SDR, SIR and SAR in dB of `estimation` against `reference`
    (module_mir_eval.py:5-91).

    `reference` (K, N) holds the K true sources, `estimation` (K, N) or (K + 1, N) the
    estimates; the extra one is the noise estimate, which takes part in the search for the
    assignment -- a speaker confused with the noise is found -- and is then left out.  With
    further axes, `(K, D, ..., N)` against `(K [+ 1], D, ..., N)`, every index of the axes
    between the first and the last is a problem of its own; all of them are one batched call.
    1 <= K, estimates <= 8, 1 <= filter_length <= 512 (512 is what `mir_eval` uses).

    Returns (sdr, sir, sar, selection), each of shape (K, ...): `selection[k]` is the estimate
    assigned to source k, picked to maximise the mean SIR.  `compute_permutation=False`
    compares estimate k with source k and returns (sdr, sir, sar); it needs as many estimates
    as sources (NotImplementedError otherwise).  `return_dict=True` returns a dict with these
    names as keys.  Misfit shapes raise ValueError, and so does an all-zero source or estimate.

    NumPy in gives NumPy out; a device tensor (float32 or float64) gives float64 / int64
    tensors on its device.
    """
    values, selection, K, mid, like_torch, home = _evaluate(
        reference, estimation, compute_permutation, filter_length)
    # (B, K) -> (K, *mid)
    sdr, sir, sar = (_signals.result(v.transpose(0, 1).reshape((K,) + mid), like_torch, home)
                     for v in values)
    if compute_permutation:
        selection = _signals.result(selection.transpose(0, 1).reshape((K,) + mid), like_torch,
                                    home)
        if return_dict:
            return {'sdr': sdr, 'sir': sir, 'sar': sar, 'selection': selection}
        return sdr, sir, sar, selection
    if return_dict:
        return {'sdr': sdr, 'sir': sir, 'sar': sar}
    return sdr, sir, sar
