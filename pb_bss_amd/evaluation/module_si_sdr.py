"""Scale-invariant SDR (reference: pb_bss/evaluation/module_si_sdr.py) on the device.

One call into csrc/eval.hip (`pbbss_si_sdr`): a Gram pass over the rows, a residual pass with the
optimal scaling of the finished Gram pass, float64 throughout.  NumPy in (float64, as the
reference asserts) gives NumPy out; a device tensor (float32 or float64, widened in registers)
gives a float64 tensor on the same device, enqueued on the current stream without a host
synchronisation.
"""
import numpy as np

from .. import _lib
from . import _signals
from ._signals import SPAN  # noqa: F401  (samples per workgroup; the tests name it)

_MAX_ROWS = 8  # rows of each argument a lane keeps in registers (csrc/eval.hpp: kEvalMaxRows)


def _launch(ref, est, B, Kr, Ke, N, strides, out):
    t = _lib.torch()
    _lib.launch('pbbss_si_sdr', ref.device, _lib.view_ptr(ref), _lib.view_ptr(est),
                ref.dtype == t.float64, B, Kr, Ke, N, *strides, out,
                what=f'si_sdr(B={B}, Kr={Kr}, Ke={Ke}, N={N})')


def _unit_last_axis(x, N):
    return x if N == 1 or x.stride(-1) == 1 else x.contiguous()


def si_sdr(reference, estimation):
    """Scale-invariant SDR in dB of `estimation` against `reference`
    (module_si_sdr.py:4-56): the estimate is split into its projection onto the reference and
    the rest, and the result is the energy of the first over the energy of the second.  The
    samples run along the last axis of both arguments.

    float64, of the shape the two arguments broadcast to without the sample axis.  A zero
    reference or a zero estimate gives nan, an estimate that is an exact multiple of the
    reference inf, as in the reference.

    The two arguments broadcast against each other.  Two forms are read in place, every row
    once: same-shaped arguments (one pair per row; an argument broadcast over all rows
    included), and the outer form `reference (..., Kr, 1, T)` against `estimation (..., 1, Ke,
    T)` or its transpose with at most 8 rows on either side -- the (Kr, Ke) score matrix that
    resolves a permutation.  Anything else, and a last axis with a stride other than one, takes
    one copy.
    """
    like_torch, home = _signals.home_of(reference, estimation)
    if not _lib.is_torch(reference):
        reference = np.asarray(reference)
        if not like_torch:
            assert reference.dtype == np.float64, reference.dtype
    if not _lib.is_torch(estimation):
        estimation = np.asarray(estimation)
        if not like_torch:
            assert estimation.dtype == np.float64, estimation.dtype
    t = _lib.require_gpu()
    ref = _signals.device_signal(reference, complex_ok=False)
    est = _signals.device_signal(estimation, complex_ok=False)
    if est.device != ref.device:
        est = est.to(ref.device)
    ref, est = _signals.common_dtype(ref, est)
    if ref.dim() == 0 or est.dim() == 0:
        raise ValueError('si_sdr needs a sample axis')
    shape = tuple(t.broadcast_shapes(ref.shape, est.shape))
    N = shape[-1]
    lead = shape[:-1]
    if N == 0:
        raise ValueError(f'empty signal: shape {shape}')
    out_numel = int(np.prod(lead, dtype=np.int64))
    if out_numel == 0:
        return _signals.result(t.empty(lead, dtype=t.float64, device=ref.device), like_torch, home)

    def broadcast(x):
        if x.shape[-1] == N:
            x = _unit_last_axis(x, N)
        x = x.expand(shape)
        return _unit_last_axis(x, N)  # a broadcast sample axis is written out

    rb, eb = broadcast(ref), broadcast(est)
    axes = [(lead[a], rb.stride(a), eb.stride(a)) for a in range(len(lead))]

    def batch_of(merged):
        if len(merged) > 1:
            return None
        return merged[0] if merged else (1, 0, 0)

    batch = batch_of(_signals.collapse(axes))
    if batch is not None:  # one pair per row
        B, rs, es = batch
        out = t.empty((B, 1, 1), dtype=t.float64, device=ref.device)
        _launch(rb, eb, B, 1, 1, N, (rs, 0, es, 0), out)
        return _signals.result(out.reshape(lead), like_torch, home)

    if len(lead) >= 2:  # outer form
        (s1, r1, e1), (s2, r2, e2) = axes[-2], axes[-1]
        batch = batch_of(_signals.collapse(axes[:-2]))
        plain = r2 == 0 and e1 == 0    # reference (..., Kr, 1, T), estimation (..., 1, Ke, T)
        swapped = r1 == 0 and e2 == 0  # reference (..., 1, Kr, T), estimation (..., Ke, 1, T)
        if batch is not None and (plain or swapped) and max(s1, s2) <= _MAX_ROWS:
            B, rs, es = batch
            if plain:
                Kr, Ke, rr, er = s1, s2, r1, e2
            else:
                Kr, Ke, rr, er = s2, s1, r2, e1
            out = t.empty((B, Kr, Ke), dtype=t.float64, device=ref.device)
            _launch(rb, eb, B, Kr, Ke, N, (rs, rr, es, er), out)
            if swapped:
                out = out.transpose(1, 2)
            return _signals.result(out.reshape(lead), like_torch, home)

    # neither form: the broadcast pairs written out, one pair per row
    rb, eb = rb.contiguous(), eb.contiguous()
    out = t.empty((out_numel, 1, 1), dtype=t.float64, device=ref.device)
    _launch(rb, eb, out_numel, 1, 1, N, (N, 0, N, 0), out)
    return _signals.result(out.reshape(lead), like_torch, home)
