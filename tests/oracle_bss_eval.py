"""Float64 yardstick for BSS-Eval SDR / SIR / SAR (Vincent et al. 2006, BSS Eval 3.0: the
decomposition `mir_eval.separation.bss_eval_sources` computes and the K+1 variant of
pb_bss/evaluation/module_mir_eval.py:94-141), restated in NumPy because the package itself is
not installed.  Two independent routes:

  direct   the explicit (N + L - 1) x (K L) matrix of delayed references and
           `numpy.linalg.lstsq` on it -- the definition of the projection;
  normal   correlations by FFT, the block-Toeplitz normal equations, `solve` and `lstsq` on
           LinAlgError, the filters applied by convolution -- the way the package computes it.

The estimate, zero-padded to N + L - 1 samples, is projected onto the L delays of reference j
(P_j) and onto the L delays of all K references (P_all):
    SDR = |P_j|^2 / |e - P_j|^2,  SIR = |P_j|^2 / |P_all - P_j|^2,  SAR = |P_all|^2 / |e - P_all|^2
in dB.  The selection maximises the mean SIR over the ordered picks of K of the Ke estimates,
the first in `itertools.permutations` order among equals.

Also the seeded generators of the cases the CPU and GPU tests share, and `load_reference`.
"""
import importlib.util
import itertools
import os

import numpy as np

FILTER_LENGTH = 512
# the recorded answer of the real package: OutputMetrics doctest, pb_bss/evaluation/wrapper.py
DOCTEST = {
    'sdr': np.array([7.2565, 7.3303]),
    'sir': np.array([25.6896, 46.638]),
    'sar': np.array([7.3309, 7.3309]),
    'selection': np.array([0, 1]),
}


def doctest_signals():
    """(speech_source, speech_prediction) of that doctest"""
    prediction = np.array([[1., 2., 3., 4.] * 1000, [4., 3., 2., 1.] * 1000])
    source = np.array([[1., 2., 2., 3., 2.] * 800, [4., 3., 3., 2., 3.] * 800])
    return source, prediction


def load_reference():
    """(module_mir_eval, wrapper) of the unmodified reference, loaded by path with stand-ins for
    the packages `wrapper` imports at its top and that are not installed"""
    import sys
    import types
    from oracle import refshim
    root = os.path.join(refshim.REFERENCE_ROOT, 'pb_bss', 'evaluation')
    stand_ins = {}
    for name in ('cached_property', 'einops', 'pb_bss'):
        if name not in sys.modules:
            stand_ins[name] = types.ModuleType(name)
    if 'cached_property' in stand_ins:
        import functools
        stand_ins['cached_property'].cached_property = functools.cached_property
    if 'einops' in stand_ins:
        stand_ins['einops'].rearrange = None
    sys.modules.update(stand_ins)
    try:
        modules = []
        for name in ('module_mir_eval', 'wrapper'):
            spec = importlib.util.spec_from_file_location(f'_reference_{name}',
                                                          os.path.join(root, name + '.py'))
            module = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(module)
            modules.append(module)
    finally:
        for name in stand_ins:
            sys.modules.pop(name, None)
    return modules


# ---- the decomposition ------------------------------------------------------------------------
def delay_matrix(references, L):
    """(N + L - 1, K L): column i L + l is reference i delayed by l samples"""
    K, N = references.shape
    A = np.zeros((N + L - 1, K * L))
    for i in range(K):
        for l in range(L):
            A[l:l + N, i * L + l] = references[i]
    return A


def _db(num, den):
    with np.errstate(divide='ignore', invalid='ignore'):
        return 10 * np.log10(num / den) if den != 0 else np.inf


def _criteria(e, p_j, p_all):
    s = np.sum(p_j ** 2)
    return (_db(s, np.sum((e - p_j) ** 2)), _db(s, np.sum((p_all - p_j) ** 2)),
            _db(np.sum(p_all ** 2), np.sum((e - p_all) ** 2)))


def _padded(estimation, L):
    return np.concatenate([estimation, np.zeros(L - 1)])


def tables_direct(references, estimations, L=FILTER_LENGTH, pairs=None):
    """(3, Ke, K) table of SDR, SIR, SAR of every estimate against every reference by the direct
    route; `pairs` restricts it to some (e, j) (the rest is NaN)"""
    references = np.asarray(references, np.float64)
    estimations = np.asarray(estimations, np.float64)
    K, Ke = len(references), len(estimations)
    A = delay_matrix(references, L)
    E = np.stack([_padded(e, L) for e in estimations], axis=1)
    p_all = A @ np.linalg.lstsq(A, E, rcond=None)[0]
    out = np.full((3, Ke, K), np.nan)
    for j in range(K):
        Aj = A[:, j * L:(j + 1) * L]
        p_j = Aj @ np.linalg.lstsq(Aj, E, rcond=None)[0]
        for e in range(Ke):
            if pairs is None or (e, j) in pairs:
                out[:, e, j] = _criteria(E[:, e], p_j[:, e], p_all[:, e])
    return out


def correlations(references, estimation, L):
    """G (K L, K L) and D (K L) of the normal equations, through FFTs of length >= N + L - 1"""
    K, N = references.shape
    n_fft = int(2 ** np.ceil(np.log2(N + L - 1.)))
    sf = np.fft.fft(references, n=n_fft, axis=1)
    sef = np.fft.fft(estimation, n=n_fft)
    G = np.zeros((K * L, K * L))
    lag = np.arange(L)
    for i in range(K):
        for j in range(i, K):
            c = np.real(np.fft.ifft(sf[i] * np.conj(sf[j])))
            # block[l, m] = sum_n s_i[n - l] s_j[n - m] = c[(m - l) mod n_fft]
            block = c[(lag[None, :] - lag[:, None]) % n_fft]
            G[i * L:(i + 1) * L, j * L:(j + 1) * L] = block
            G[j * L:(j + 1) * L, i * L:(i + 1) * L] = block.T
    D = np.zeros(K * L)
    for i in range(K):
        c = np.real(np.fft.ifft(sf[i] * np.conj(sef)))
        D[i * L:(i + 1) * L] = c[(-lag) % n_fft]
    return G, D


def _project_normal(references, estimation, L):
    K, N = references.shape
    G, D = correlations(references, estimation, L)
    try:
        C = np.linalg.solve(G, D)
    except np.linalg.LinAlgError:
        C = np.linalg.lstsq(G, D, rcond=None)[0]
    p = np.zeros(N + L - 1)
    for i in range(K):
        p += np.convolve(C[i * L:(i + 1) * L], references[i])
    return p


def tables_normal(references, estimations, L=FILTER_LENGTH, pairs=None):
    """the same table by the normal-equation route"""
    references = np.asarray(references, np.float64)
    estimations = np.asarray(estimations, np.float64)
    K, Ke = len(references), len(estimations)
    out = np.full((3, Ke, K), np.nan)
    for e in range(Ke):
        wanted = [j for j in range(K) if pairs is None or (e, j) in pairs]
        if not wanted:
            continue
        p_all = _project_normal(references, estimations[e], L)
        for j in wanted:
            p_j = _project_normal(references[j:j + 1], estimations[e], L)
            out[:, e, j] = _criteria(_padded(estimations[e], L), p_j, p_all)
    return out


def gram_condition(references, L):
    return np.linalg.cond(correlations(np.asarray(references, np.float64),
                                       np.zeros(references.shape[-1]), L)[0])


def select(sir):
    """sir (Ke, K) -> (selection (K,) int64, margin): the ordered pick of K estimates with the
    largest mean SIR, and its lead over the second best relative to its own size"""
    Ke, K = sir.shape
    candidates = list(itertools.permutations(range(Ke), K))
    dum = np.arange(K)
    mean_sir = np.array([np.mean(sir[c, dum]) for c in candidates])
    best = int(np.argmax(mean_sir))
    rest = np.delete(mean_sir, best)
    margin = np.inf if rest.size == 0 else (mean_sir[best] - rest.max()) / abs(mean_sir[best])
    return np.array(candidates[best], dtype=np.int64), margin


def bss_eval(references, estimations, L=FILTER_LENGTH, compute_permutation=True,
             route='direct', details=None):
    """-> sdr, sir, sar (K,), selection (K,) int64.  details['tables'], details['margin']."""
    references = np.asarray(references, np.float64)
    estimations = np.asarray(estimations, np.float64)
    K = len(references)
    pairs = None if compute_permutation else {(j, j) for j in range(K)}
    tables = {'direct': tables_direct, 'normal': tables_normal}[route](
        references, estimations, L, pairs)
    if compute_permutation:
        selection, margin = select(tables[1])
    else:
        selection, margin = np.arange(K), np.inf
    if details is not None:
        details['tables'] = tables
        details['margin'] = margin
    dum = np.arange(K)
    return tables[0][selection, dum], tables[1][selection, dum], tables[2][selection, dum], \
        selection


def table_difference(a, b):
    """largest |a - b| over the finite entries; the others (inf where a denominator is exactly
    zero, NaN for skipped pairs) have to coincide"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    finite = np.isfinite(a)
    assert np.array_equal(finite, np.isfinite(b)), (a, b)
    assert np.array_equal(a[~finite], b[~finite], equal_nan=True), (a, b)
    return float(np.abs(a[finite] - b[finite]).max()) if finite.any() else 0.0


def bss_eval_channels(references, estimations, L=FILTER_LENGTH, compute_permutation=True,
                      route='direct'):
    """(K, D, N) against (Ke, D, N), every channel on its own -> three (K, D) arrays and the
    (K, D) selection"""
    D = references.shape[1]
    results = [bss_eval(references[:, d], estimations[:, d], L, compute_permutation, route)
               for d in range(D)]
    return tuple(np.stack([r[m] for r in results], axis=1) for m in range(4))


# ---- seeded cases -------------------------------------------------------------------------------
def ar1(rng, K, N, pole=0.9):
    """K rows of AR(1) noise: x[n] = pole x[n - 1] + w[n]"""
    w = rng.standard_normal((K, N))
    x = np.empty((K, N))
    state = np.zeros(K)
    for n in range(N):
        state = pole * state + w[:, n]
        x[:, n] = state
    return x


def gen_case(seed, K, Ke, N, dtype=np.float64):
    """references (K, N): AR(1) noise.  estimations (Ke, N): a diagonally dominant mix of them
    (1 on the diagonal, U(0.1, 0.3) off it) plus 0.1 * white noise, the rows shuffled."""
    rng = np.random.default_rng(seed)
    references = ar1(rng, K, N)
    mix = rng.uniform(0.1, 0.3, (Ke, K))
    mix[np.arange(K), np.arange(K)] = 1.0
    estimations = mix @ references + 0.1 * rng.standard_normal((Ke, N))
    estimations = estimations[rng.permutation(Ke)]
    return references.astype(dtype), estimations.astype(dtype)


def gen_dependent_case(seed, N=1500):
    """K = 3 with the third reference the sum of the first two: a singular Gram matrix"""
    references, estimations = gen_case(seed, 3, 3, N)
    references[2] = references[0] + references[1]
    return references, estimations
