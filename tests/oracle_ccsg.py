"""The complex circular-symmetric Gaussian in NumPy, for tests/test_ccsg_oracle.py (CPU),
tests/test_gpu_ccsg.py (GPU) and tools/make_ccsg_golden.py (fixtures):

* `fit` / `log_pdf`: float64 restatements of
  pb_bss/distribution/complex_circular_symmetric_gaussian.py (`_fit` :94-116, `log_pdf` :26-48) --
  the weighted outer-product sum as one matrix product per class, the quadratic form from one
  LU solve per covariance with all frames as right-hand sides.
* `fit_ext` / `log_pdf_ext`: the same quantities in `np.longdouble` (Cholesky written out).
* the seeded case generators and the shape lists of the GPU sweep.

Observations and saliencies are widened first (complex128 / float64): the device computes in
float64 on the exactly widened values.
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# ---- the shape lists of the GPU sweep (tests/test_ccsg_oracle.py checks what they reach) ------
D_SWEEP = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 34)
N_SWEEP = (1, 63, 64, 65, 128, 129, 256, 257)
K_SWEEP = (1, 3, 4, 5, 6, 7, 8, 9)
B_SWEEP = (1, 5)
Y_DTYPES = (np.complex64, np.complex128)
SALIENCIES = (None, np.float32, np.float64)
CONDITIONS = (1e2, 1e6, 1e10)
CONDITION_DS = (3, 8, 16, 34)


# ---- float64 restatement ------------------------------------------------------------------------
def fit(y, saliency=None):
    """y (..., N, D), saliency (..., N) or None -> covariance (..., D, D) complex128."""
    floor = np.finfo(y.dtype).tiny
    y = np.asarray(y).astype(np.complex128)
    yt = np.swapaxes(y, -1, -2)
    if saliency is None:
        return (yt @ y.conj()) / y.shape[-2]
    s = np.asarray(saliency).astype(np.float64)
    den = np.maximum(s.sum(axis=-1), floor)
    return ((s[..., None, :] * yt) @ y.conj()) / den[..., None, None]


def log_pdf(y, covariance):
    """y (..., N, D), covariance (..., D, D) -> (..., N) float64."""
    y = np.asarray(y).astype(np.complex128)
    cov = np.asarray(covariance).astype(np.complex128)
    D = cov.shape[-1]
    yt = np.swapaxes(y, -1, -2)                       # (..., D, N)
    x = np.linalg.solve(cov, yt)                      # C^-1 y, all frames at once
    quad = (yt.conj() * x).sum(axis=-2).real
    return -D * np.log(np.pi) - np.linalg.slogdet(cov)[1][..., None] - quad


# ---- extended precision ---------------------------------------------------------------------------
def fit_ext(y, saliency=None):
    floor = np.longdouble(np.finfo(y.dtype).tiny)
    y = np.asarray(y).astype(np.clongdouble)
    yt = np.swapaxes(y, -1, -2)
    if saliency is None:
        return (yt @ y.conj()) / np.longdouble(y.shape[-2])
    s = np.asarray(saliency).astype(np.longdouble)
    den = np.maximum(s.sum(axis=-1), floor)
    return ((s[..., None, :] * yt) @ y.conj()) / den[..., None, None]


def cholesky_ext(cov):
    """Lower Cholesky factor of (..., D, D) Hermitian matrices in longdouble (the lower triangle
    and the real diagonal are read)."""
    a = np.asarray(cov).astype(np.clongdouble)
    D = a.shape[-1]
    L = np.zeros_like(a)
    for j in range(D):
        s = a[..., j, j].real - (np.abs(L[..., j, :j]) ** 2).sum(axis=-1)
        L[..., j, j] = np.sqrt(s)
        for i in range(j + 1, D):
            v = a[..., i, j] - (L[..., i, :j] * L[..., j, :j].conj()).sum(axis=-1)
            L[..., i, j] = v / L[..., j, j]
    return L


def log_pdf_ext(y, covariance):
    """(log_pdf (..., N), log_det (...)) in longdouble; independent axes broadcast like
    `log_pdf`."""
    y = np.asarray(y).astype(np.clongdouble)
    L = cholesky_ext(covariance)
    D = L.shape[-1]
    lead = np.broadcast_shapes(y.shape[:-2], L.shape[:-2])
    y = np.broadcast_to(y, (*lead, *y.shape[-2:]))
    L = np.broadcast_to(L, (*lead, D, D))
    z = np.zeros(y.shape, np.clongdouble)
    for j in range(D):
        acc = y[..., :, j] - (L[..., None, j, :j] * z[..., :, :j]).sum(axis=-1)
        z[..., :, j] = acc / L[..., None, j, j]
    quad = (np.abs(z) ** 2).sum(axis=-1)
    log_det = 2 * np.log(np.diagonal(L, axis1=-2, axis2=-1).real).sum(axis=-1)
    pi = np.longdouble('3.14159265358979323846264338327950288')
    return -D * np.log(pi) - log_det[..., None] - quad, log_det


# ---- seeded generators ------------------------------------------------------------------------------
def frames(seed, shape, dtype=np.complex128):
    """Circular complex normal frames of unit variance, rounded to `dtype`."""
    rng = np.random.RandomState(seed)
    y = (rng.normal(size=shape) + 1j * rng.normal(size=shape)) / np.sqrt(2)
    return y.astype(dtype)


def saliency(seed, shape, dtype=np.float64):
    return np.random.RandomState(seed + 1000).uniform(0.05, 1.0, size=shape).astype(dtype)


def spd(seed, lead, D, cond=1e2):
    """Hermitian positive definite (..., D, D) of condition `cond`: Q diag(logspace) Q^H with a
    random unitary Q, the largest eigenvalue 1; exactly Hermitian with a real diagonal."""
    rng = np.random.RandomState(seed + 2000)
    g = rng.normal(size=(*lead, D, D)) + 1j * rng.normal(size=(*lead, D, D))
    q, _ = np.linalg.qr(g)
    lam = np.logspace(0, -np.log10(cond), D) if D > 1 else np.ones(1)
    c = (q * lam) @ np.swapaxes(q.conj(), -1, -2)
    return (c + np.swapaxes(c.conj(), -1, -2)) / 2


def conditioned(cond, D, N=64, seed=7):
    """(y (N, D) drawn from C, C (D, D)) with cond(C) = `cond`."""
    c = spd(seed + D, (), D, cond)
    y = frames(seed + D + 1, (N, D)) @ np.linalg.cholesky(c).T
    return y, c


def sweep_cases(D):
    """The (N, K, B, y dtype, saliency kind) combinations the GPU sweep runs at sensor count D:
    every N of N_SWEEP and every K of K_SWEEP, the other axes cycling so that each of their
    values meets every D."""
    cases = []
    for i, N in enumerate(N_SWEEP):
        cases.append((N, K_SWEEP[(i + D) % len(K_SWEEP)], B_SWEEP[(i + D) % 2],
                      Y_DTYPES[i % 2], SALIENCIES[(i + D) % 3]))
    for i, K in enumerate(K_SWEEP):
        cases.append((65 + 64 * (i % 2), K, B_SWEEP[(i + D + 1) % 2], Y_DTYPES[(i + 1) % 2],
                      SALIENCIES[1 + (i + D) % 2]))
    return cases


def case(D, N, K, B, y_dtype, sal_dtype):
    """Inputs of one sweep case: y (B, N, D), saliency (B, K, N) or None (the fit then has one
    class), covariance (B, K, D, D) (well-conditioned, drawn independently of y, for the
    log-pdf)."""
    seed = 1 + D + 37 * N + 101 * K + 7 * B
    y = frames(seed, (B, N, D), y_dtype)
    s = None if sal_dtype is None else saliency(seed, (B, K, N), sal_dtype)
    return y, s, spd(seed, (B, K), D)


def oracle_fit(y, s, fit_fn=fit):
    """`fit_fn` on the arrays of `case` -> (B, K, D, D) (K = 1 without saliency)."""
    return fit_fn(y)[:, None] if s is None else fit_fn(y[:, None], s)


# ---- fixtures (written by tools/make_ccsg_golden.py from the live reference) ---------------------------
FIXTURE_CASES = tuple((D,) + c for D in (1, 3, 8, 9) for c in sweep_cases(D) if c[0] <= 65)
SAMPLE_SEED, SAMPLE_SIZE, SAMPLE_D = 5, (6,), 4


def case_key(D, N, K, B, y_dtype, sal_dtype):
    sal = 'none' if sal_dtype is None else np.dtype(sal_dtype).name
    return f'D{D}_N{N}_K{K}_B{B}_{np.dtype(y_dtype).name}_{sal}'


@functools.lru_cache(maxsize=None)
def fixtures():
    """{array name: array} of tests/golden/ccsg_reference.npz."""
    with np.load(os.path.join(GOLDEN, 'ccsg_reference.npz')) as f:
        return {k: f[k] for k in f.files}


def sample_covariance():
    return spd(SAMPLE_SEED, (), SAMPLE_D)
