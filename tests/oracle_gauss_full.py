"""Inputs and an extended-precision reference for the full-covariance Gaussian kernels
(csrc/gauss_full.hip): NumPy only.

`fit_ext` / `log_pdf_ext` restate `oracle.embed.gaussian_fit(..., 'full')` and
`gaussian_log_pdf(..., 'full')` in `np.longdouble` (64-bit mantissa on x86-64) with a
hand-written Cholesky and forward substitution.  The log-pdf is the one the reference writes:
`white = P d` with `P = L^-T` -- NOT the textbook Mahalanobis form `L^-1 d`; with X = L^-1 the
quadratic form is that of `X X^T`, not of `cov^-1 = X^T X`.  tests/test_gauss_full_oracle.py
shows that the float64 oracle stays within 1e-13 of this reference on every hard input below,
which is what lets the GPU tests use the (fast) float64 oracle as their reference.

The hard inputs.  A "spread" is the standard deviation of the cloud, about 1 here.
  off_centre   one row lies `dist` spreads from the cloud and carries weight 0 or 1e-12; it is
               row 0 (the point the single-pass M-steps used to centre on) or the last row
  separated    two clusters `delta` spreads apart, one class each, row 0 in the first
  offset       every row at 1e6 +- 1
  scaled       the cloud times 1e100 / 1e-100
  conditioned  cond(cov) = 1e6 / 1e10
  empty        one class with all-zero weight
  nan_row      a NaN in a row of weight zero

Layout as in oracle/embed.py: y (N, E), weights (K, N).
"""
import functools

import numpy as np

__all__ = ['E_SWEEP', 'chol_positions', 'tiles', 'cloud', 'off_centre', 'separated', 'offset',
           'conditioned', 'scaled', 'empty_class', 'nan_row', 'hard_cases', 'fit_ext', 'log_pdf_ext',
           'logpdf_blocks']

LD = np.longdouble

# gf_chol_inverse compiles one variant per Q = ceil(E (E + 1) / 2 / 256): both sides of every
# boundary (22|23, 31|32, 38|39, 44|45, 50|51, 54|55, 59|60), the tile counts ceil((E + 1) / 16)
# with E + 1 exact (15, 31, 47, 63) and one over (16, 32, 48), and E < 5.
E_SWEEP = (1, 2, 3, 4, 15, 16, 22, 23, 31, 32, 38, 39, 44, 45, 47, 48, 50, 51, 54, 55, 59, 60,
           62, 63)


def chol_positions(E):
    """Q of gf_chol_inverse: lower-triangle positions per thread of a 256-thread workgroup."""
    return (E * (E + 1) // 2 + 255) // 256


def tiles(E):
    """16-blocks of the augmented vector [y - c; 1]."""
    return (E + 1 + 15) // 16


def logpdf_blocks(K):
    """S of gf_logpdf_go: samples per workgroup, 64 * groups."""
    return 64 * max(1, min(8, (32 * 1024) // (8 * 64 * K)))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def cloud(N, E, seed=0, cond=1e2):
    """(N, E) rows with covariance of condition number ~cond, largest variance ~1, mean O(1)."""
    rng = np.random.default_rng([seed, N, E])
    q, _ = np.linalg.qr(rng.normal(size=(E, E)))
    s = np.sqrt(cond) ** (-np.arange(E) / max(E - 1, 1))
    return rng.normal(size=(N, E)) * s @ q.T + rng.normal(size=E)


def _weights(K, N, seed):
    return np.random.default_rng([seed, K, N, 7]).uniform(size=(K, N)) ** 2


@functools.lru_cache(maxsize=None)
def off_centre(dist, weight, where='first', N=300, E=15, K=2, seed=1):
    """One row `dist` spreads from the cloud with `weight` in every class, at row 0 or last."""
    y = cloud(N, E, seed)
    w = _weights(K, N, seed)
    u = np.random.default_rng(seed + 5).normal(size=E)
    u /= np.linalg.norm(u)
    y[0] = y[1:].mean(0) + dist * u
    w[:, 0] = weight
    if where == 'last':
        y = np.roll(y, -1, axis=0)
        w = np.roll(w, -1, axis=1)
    return _frozen(y, w)


@functools.lru_cache(maxsize=None)
def separated(delta, N=300, E=15, seed=2):
    """Two clusters `delta` spreads apart; class k selects cluster k; row 0 is in cluster 0.
    Returns y, weights and the labels."""
    y = cloud(N, E, seed)
    lab = (np.arange(N) % 3 == 1).astype(int)  # row 0 -> cluster 0, a third of the rows -> 1
    u = np.random.default_rng(seed + 5).normal(size=E)
    u /= np.linalg.norm(u)
    y = y + delta * lab[:, None] * u
    w = _weights(2, N, seed) * (lab[None, :] == np.arange(2)[:, None])
    return _frozen(y, w, lab)


@functools.lru_cache(maxsize=None)
def offset(N=300, E=15, K=2, seed=3):
    """Every row at 1e6 +- 1."""
    rng = np.random.default_rng(seed)
    return _frozen(1e6 + rng.uniform(-1.0, 1.0, size=(N, E)), _weights(K, N, seed))


@functools.lru_cache(maxsize=None)
def conditioned(cond, N=300, E=15, K=2, seed=4):
    return _frozen(cloud(N, E, seed, cond), _weights(K, N, seed))


@functools.lru_cache(maxsize=None)
def scaled(factor, N=300, E=15, K=2, seed=4):
    """The cond(cov) = 1e2 cloud times `factor`."""
    y, w = conditioned(1e2, N, E, K, seed)
    return _frozen(y * factor, w)


@functools.lru_cache(maxsize=None)
def empty_class(N=300, E=15, seed=5):
    w = _weights(2, N, seed)
    w[1] = 0.0
    return _frozen(cloud(N, E, seed), w)


@functools.lru_cache(maxsize=None)
def nan_row(row, N=300, E=15, seed=6):
    """NaN in one entry of a row whose weight is zero in every class."""
    y = cloud(N, E, seed)
    w = _weights(2, N, seed)
    y[row, 3] = np.nan
    w[:, row] = 0.0
    return _frozen(y, w)


def hard_cases():
    """name -> (y, weights): every finite hard input of the GPU tests."""
    out = {}
    for dist in (1e2, 1e4, 1e6):
        for weight in (0.0, 1e-12):
            for where in ('first', 'last'):
                out[f'off_centre_{dist:g}_{weight:g}_{where}'] = off_centre(dist, weight, where)
    for delta in (1e2, 1e4):
        out[f'separated_{delta:g}'] = separated(delta)[:2]
    out['offset_1e6'] = offset()
    for factor in (1e100, 1e-100):
        out[f'scaled_{factor:g}'] = scaled(factor)
    for cond in (1e6, 1e10):
        out[f'conditioned_{cond:g}'] = conditioned(cond)
    out['empty_class'] = empty_class()
    return out


# ---------------------------------------------------------------- extended precision
def fit_ext(y, weights):
    """oracle.embed.gaussian_fit(y[None], weights, 'full') in longdouble: (K, E), (K, E, E)."""
    y = np.asarray(y, dtype=LD)
    w = np.asarray(weights, dtype=LD)
    den = np.maximum(w.sum(-1), LD(np.finfo(np.float64).tiny))
    mean = (w @ y) / den[:, None]
    diff = y[None] - mean[:, None, :]
    cov = np.einsum('kn,knd,knD->kdD', w, diff, diff) / den[:, None, None]
    return mean, cov


def cholesky_ext(a):
    """Lower Cholesky factor of one (E, E) longdouble matrix, row by row."""
    E = a.shape[0]
    l = np.zeros((E, E), dtype=LD)
    for i in range(E):
        for j in range(i):
            l[i, j] = (a[i, j] - l[i, :j] @ l[j, :j]) / l[j, j]
        d = a[i, i] - l[i, :i] @ l[i, :i]
        if not d > 0:
            raise np.linalg.LinAlgError('not positive definite')
        l[i, i] = np.sqrt(d)
    return l


def lower_inverse_ext(l):
    """X = L^-1 by forward substitution on the identity."""
    E = l.shape[0]
    x = np.zeros((E, E), dtype=LD)
    for i in range(E):
        x[i, i] = 1 / l[i, i]
        x[i, :i] = -(l[i, :i] @ x[:i, :i]) / l[i, i]
    return x


def log_pdf_ext(y, mean, covariance):
    """oracle.embed.gaussian_log_pdf(y[None], mean, covariance, 'full') in longdouble, from the
    float64 model the oracle is given: (K, N).  white = P d with P = L^-T, as the reference."""
    y = np.asarray(y, dtype=LD)
    mean = np.asarray(mean, dtype=LD)
    covariance = np.asarray(covariance, dtype=LD)
    K, E = mean.shape
    out = np.empty((K, y.shape[0]), dtype=LD)
    for k in range(K):
        p = lower_inverse_ext(cholesky_ext(covariance[k])).T
        white = (y - mean[k]) @ p.T  # white[n, i] = sum_j P[i, j] d[n, j]
        out[k] = (-LD(0.5) * E * np.log(2 * LD(np.pi)) + np.log(np.diagonal(p)).sum()
                  - LD(0.5) * (white * white).sum(-1))
    return out
