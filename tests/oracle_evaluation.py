"""Float64 restatement of the reference's NumPy metrics (pb_bss/evaluation/module_si_sdr.py and
sxr_module.py): `si_sdr`, `get_snr`, `input_sxr`, `output_sxr`, with leading batch axes, the
selection `output_sxr` finds and how well determined it is.

Also the seeded generators of the cases the CPU and GPU tests share, and `load_reference`, which
loads the two reference files by path (the reference package's __init__ imports packages that
are not installed).
"""
import collections
import importlib.util
import itertools
import os

import numpy as np

SI_SDR_NAMES = ['si_sdr']
SXR_NAMES = ['get_snr', 'input_sxr', 'output_sxr']  # sxr_module.__all__ of the reference
SXR = collections.namedtuple('SXR', ['sdr', 'sir', 'snr'])
MARGIN = 1e-6  # relative lead the best selection needs over the second best


def load_reference():
    """(module_si_sdr, sxr_module) of the unmodified reference"""
    from oracle import refshim
    root = os.path.join(refshim.REFERENCE_ROOT, 'pb_bss', 'evaluation')
    modules = []
    for name in ('module_si_sdr', 'sxr_module'):
        spec = importlib.util.spec_from_file_location(f'_reference_{name}',
                                                      os.path.join(root, name + '.py'))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        modules.append(module)
    return modules


# ---- the metrics ----------------------------------------------------------------------------
def si_sdr(reference, estimation):
    e, r = np.broadcast_arrays(np.asarray(estimation, np.float64),
                               np.asarray(reference, np.float64))
    with np.errstate(divide='ignore', invalid='ignore'):
        alpha = np.sum(r * e, axis=-1, keepdims=True) / np.sum(r ** 2, axis=-1, keepdims=True)
        target = alpha * r
        residual = e - target
        return 10 * np.log10(np.sum(target ** 2, axis=-1) / np.sum(residual ** 2, axis=-1))


def power(x, axis=None, keepdims=False):
    x = np.asarray(x)
    if np.iscomplexobj(x):
        x = x.astype(np.complex128)
        return np.mean(x.real ** 2 + x.imag ** 2, axis=axis, keepdims=keepdims)
    return np.mean(x.astype(np.float64) ** 2, axis=axis, keepdims=keepdims)


def get_snr(X, N, axis=None, keepdims=False):
    with np.errstate(divide='ignore', invalid='ignore'):
        return 10 * np.log10(power(X, axis, keepdims) / power(N, axis, keepdims))


def _db(s, x):
    with np.errstate(divide='ignore', invalid='ignore'):
        return 10 * np.log10(s / x)


def _input_sxr_one(images, noise, average_sources, average_channels):
    K, D, _ = images.shape
    S = power(images, -1)
    N = power(noise, -1)
    I = np.zeros((K, D))
    for k in range(K):
        for d in range(D):
            I[k, d] = np.sum(S[[n for n in range(K) if n != k], d], axis=0)
    if average_channels:
        S, I, N = (np.mean(p, axis=-1) for p in (S, I, N))
    values = [_db(S, I + N), _db(S, I), _db(S, N)]
    if average_sources:
        values = [np.mean(v, axis=0) for v in values]
    return values


def _stack(items):
    """list over the flattened batch of [sdr, sir, snr] -> three arrays (batch, ...)"""
    return [np.array([item[m] for item in items]) for m in range(3)]


def input_sxr(images, noise, average_sources=True, average_channels=True):
    images, noise = np.asarray(images), np.asarray(noise)
    batch = images.shape[:-3]
    assert noise.shape[:-2] == batch and noise.shape[-2:] == images.shape[-2:]
    im = images.reshape((-1,) + images.shape[-3:])
    no = noise.reshape((-1,) + noise.shape[-2:])
    items = [_input_sxr_one(a, b, average_sources, average_channels) for a, b in zip(im, no)]
    return SXR(*[v.reshape(batch + v.shape[1:]) for v in _stack(items)])


def _output_sxr_one(contribution, noise, average_sources):
    Ks, Kt, _ = contribution.shape
    S = power(contribution, -1)
    N = power(noise, -1)
    selections = list(itertools.permutations(range(Kt), Ks))
    totals = np.array([np.sum([S[k, sel[k]] for k in range(Ks)]) for sel in selections])
    best = int(np.argmax(totals))
    sel = np.array(selections[best], dtype=np.int64)
    rest = np.delete(totals, best)
    margin = np.inf if rest.size == 0 else (totals[best] - rest.max()) / totals[best]
    SS = np.array([S[k, sel[k]] for k in range(Ks)])
    II = np.array([np.sum(np.delete(S[:, sel[k]], k)) for k in range(Ks)])
    NN = N[sel]
    values = [_db(SS, II + NN), _db(SS, II), _db(SS, NN)]
    if average_sources:
        values = [np.mean(v) for v in values]
    return values, sel, margin


def output_sxr(contribution, noise, average_sources=True, details=None):
    """-> (SXR, selection (..., Ks) int64).  details['margin']: per batch item, the relative
    lead of the best mutual power over the second best (inf where there is one selection)."""
    contribution, noise = np.asarray(contribution), np.asarray(noise)
    batch = contribution.shape[:-3]
    assert noise.shape[:-2] == batch and noise.shape[-2:] == contribution.shape[-2:]
    co = contribution.reshape((-1,) + contribution.shape[-3:])
    no = noise.reshape((-1,) + noise.shape[-2:])
    items = [_output_sxr_one(a, b, average_sources) for a, b in zip(co, no)]
    values = _stack([item[0] for item in items])
    sel = np.array([item[1] for item in items]).reshape(batch + (contribution.shape[-3],))
    if details is not None:
        details['margin'] = np.array([item[2] for item in items]).reshape(batch)
    return SXR(*[v.reshape(batch + v.shape[1:]) for v in values]), sel


# ---- seeded cases ---------------------------------------------------------------------------
def gen_signals(seed, shape, dtype=np.float64):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == 'c':
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
    return rng.standard_normal(shape).astype(dtype)


def gen_si_sdr(seed, shape, snr_db=10.0, dtype=np.float64):
    """reference and estimation = gain * reference + noise at about `snr_db`"""
    rng = np.random.default_rng(seed)
    reference = rng.standard_normal(shape)
    gain = rng.uniform(0.5, 2.0, shape[:-1] + (1,))
    estimation = gain * reference + 10 ** (-snr_db / 20) * rng.standard_normal(shape)
    return reference.astype(dtype), estimation.astype(dtype)


def gen_output_case(seed, batch, Ks, Kt, N, dtype=np.float64):
    """contributions (*batch, Ks, Kt, N), noise (*batch, Kt, N): every source is strong in one
    output of its own, drawn per batch item, and leaks into the others."""
    rng = np.random.default_rng(seed)
    B = int(np.prod(batch, dtype=np.int64))
    gain = np.empty((B, Ks, Kt))
    for b in range(B):
        home = rng.permutation(Kt)[:Ks]
        gain[b] = rng.uniform(0.1, 0.4, (Ks, Kt))
        gain[b, np.arange(Ks), home] = rng.uniform(1.0, 2.0, Ks)
    gain = gain.reshape(tuple(batch) + (Ks, Kt, 1))
    contribution = gain * gen_signals(rng.integers(1 << 30), tuple(batch) + (Ks, Kt, N), dtype)
    noise = 0.2 * gen_signals(rng.integers(1 << 30), tuple(batch) + (Kt, N), dtype)
    return contribution.astype(dtype), noise.astype(dtype)


def gen_input_case(seed, batch, K, D, N, dtype=np.float64):
    rng = np.random.default_rng(seed)
    gain = rng.uniform(0.3, 2.0, tuple(batch) + (K, D, 1))
    images = gain * gen_signals(rng.integers(1 << 30), tuple(batch) + (K, D, N), dtype)
    noise = 0.3 * gen_signals(rng.integers(1 << 30), tuple(batch) + (D, N), dtype)
    return images.astype(dtype), noise.astype(dtype)
