"""Inputs for the per-bin von-Mises-Fisher mixture kernel (csrc/vmf_bin.hip) whose concentrations
sit where the test wants them, and probe rows that make the normaliser visible (NumPy float64
and oracle/embed.py only).

The kernel's hand-written numerics -- the tabulated log-Bessel polynomial, its block size, the
clamp of the concentration -- depend on `max_concentration` / `min_concentration` and on which
side of them a class lands.  `scenario` draws 16 small mixtures with a noise level per class;
with a hard one-hot initialisation the raw concentration (Banerjee 2005 eq. 4.4, unclipped) of a
class with noise sigma is about 1 / sigma^2, so a noise level chooses the side of a clamp.  (Soft
0.9 / 0.1 labels would cap a tight class near 50: a tenth of the other class's spread rows is
enough -- tests/test_vmf_bin_oracle.py shows it.)

The normaliser is no output of the kernel.  `with_probes` appends rows with saliency 0 -- the
M-step does not see them, the final E-step does -- on the great circle from mean 0 towards mean 1,
between the angles where the oracle's posterior of class 0 crosses 0.95 and 0.05.  There
d gamma / d logit = gamma (1 - gamma) >= 0.0475, at most 1/4: an error delta in offset_0 -
offset_1 moves the posterior by up to delta / 4, instead of vanishing in a saturated 0 or 1.

`case` builds a named scenario with its probes and the oracle's one-iteration result, once per
(name, parameter, E, dtype); the arrays are read-only and shared between the tests.

Layout as in oracle/embed.py: y (B, N, E), init (B, K, N), saliency (B, N).
"""
import functools

import numpy as np

from oracle import embed as oe

__all__ = ['B', 'E_LIST', 'CASES', 'scenario', 'with_probes', 'raw_concentration', 'logit',
           'probe_angles', 'case', 'tune_sigma', 'edge_rows']

B = 16                       # the smallest batch embed_mixture_path sends to the per-bin route
E_LIST = (2, 3, 4, 8, 12, 13, 16)   # nu = 0, 1/2, the largest order; 13: a padded EP = 16
N_ROWS, N_PROBES = 300, 64

# name -> list of (parameter, spec).  spec: sigma per class (a number, or a function of E),
# clamps, and what is promised of each class's RAW concentration: 'high' (above the cap),
# 'low' (below the floor), 'free' (between them) -- each by 3 % at least.  `target`: class 0's
# noise is tuned per mixture until its raw concentration is this value.
_HIGH = dict(sigma=(0.01, 0.8), cmin=1e-10, promise=('high', 'free'))
CASES = {
    # block size of the tabulated polynomial, bR = ceil((ceil(cmax) + 48) / 64): 1, 2, 9, 10, 16
    'clamped_high': [(c, dict(_HIGH, cmax=float(c))) for c in (10, 80, 500, 529, 960)],
    # cmax > 960: the x-sized blocks of embed_dev.hpp inside the per-bin kernel (bR = 0)
    'generic_series': [(c, dict(_HIGH, cmax=float(c))) for c in (961, 2000)],
    # the sixteen-term blocks with a concentration that is NOT the cap
    'unclamped_upper_table': [(k, dict(sigma=(k ** -0.5, 0.8), cmin=1e-10, cmax=960.0, target=float(k),
                                       promise=('free', 'free'))) for k in (600, 900)],
    'clamped_low': [(5, dict(sigma=(0.3, 3.0), cmin=5.0, cmax=500.0, promise=('free', 'low')))],
    # the noise of test_vmfmm_many_small_mixtures_persistent_kernel: 0.6 per component against
    # means of length sqrt(E)
    'mild': [(0, dict(sigma=lambda E: 0.6 / np.sqrt(E), cmin=1e-10, cmax=500.0,
                      promise=('free', 'free')))],
}


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def logit(p):
    return np.log(p) - np.log1p(-p)


def _draw(E, K, N, seed, batch):
    rng = np.random.default_rng(seed)
    if K <= E:   # orthonormal class means: the angle between two classes is a right one
        mu = np.linalg.qr(rng.standard_normal((batch, E, K)))[0].transpose(0, 2, 1)
    else:
        mu = _unit(rng.standard_normal((batch, K, E)))
    noise = rng.standard_normal((batch, N, E))
    sal = rng.uniform(0.1, 1.0, size=(batch, N))
    return np.ascontiguousarray(mu), noise, sal


def scenario(E, K, N, sigma, seed, dtype, batch=B):
    """`batch` mixtures of N rows unit(mu_k + sigma_k noise), k = n mod K, with a hard one-hot
    initialisation and a saliency uniform in [0.1, 1].  sigma: one number, K numbers, or
    (batch, K) -- one noise level per mixture and class.
    -> y (batch, N, E) of `dtype`, init (batch, K, N) float64, saliency (batch, N) float64."""
    mu, noise, sal = _draw(E, K, N, seed, batch)
    sig = np.broadcast_to(np.asarray(sigma, np.float64), (batch, K))
    lab = np.arange(N) % K
    y = _unit(mu[:, lab] + sig[:, lab, None] * noise).astype(dtype)
    init = np.zeros((batch, K, N))
    init[:, lab, np.arange(N)] = 1.0
    return y, init, sal


def raw_concentration(y, init, sal):
    """(batch, K): the concentration of the first M-step before it is clipped."""
    y = oe.unit_rows(np.asarray(y, np.float64))
    return oe.vmf_fit(y[..., None, :, :], init * sal[..., None, :], -np.inf, np.inf)[1]


def tune_sigma(E, K, N, sigma, seed, target, rounds=6):
    """(B, K) noise levels with class 0's tuned, per mixture, until its raw concentration is
    `target` (kappa ~ 1 / sigma^2: the fixed point sigma <- sigma sqrt(kappa / target))."""
    sig = np.broadcast_to(np.asarray(sigma, np.float64), (B, K)).copy()
    for _ in range(rounds):
        y, init, sal = scenario(E, K, N, sig, seed, np.float64)
        sig[:, 0] *= np.sqrt(raw_concentration(y, init, sal)[:, 0] / target)
    return sig


def _circle(mean, theta):
    """Rows (len(theta), E) on the great circle from mean[0] towards mean[1]."""
    m0 = mean[0] / np.linalg.norm(mean[0])
    u = mean[1] - (mean[1] @ m0) * m0
    if np.linalg.norm(u) < 1e-6:   # (anti)parallel means: any direction orthogonal to mean 0
        u = np.eye(len(m0))[np.argmin(np.abs(m0))]
        u = u - (u @ m0) * m0
    u /= np.linalg.norm(u)
    return np.cos(theta)[:, None] * m0 + np.sin(theta)[:, None] * u


def _crossing(model, lo, hi, level, depth=3, grid=513):
    """First angle in [lo, hi] at which the oracle's posterior of class 0 is below `level`
    (nested dense grids; hi where it never is)."""
    for _ in range(depth):
        theta = np.linspace(lo, hi, grid)
        p = oe.vmfmm_predict(model, _circle(model['mean'], theta))[0]
        below = np.nonzero(p < level)[0]
        if len(below) == 0:
            return hi
        i = below[0]
        if i == 0:
            return lo
        lo, hi = theta[i - 1], theta[i]
    return hi


def probe_angles(model, P):
    """P angles evenly spaced inside the interval between the 0.95 and the 0.05 crossing of the
    posterior of class 0 along the great circle, for ONE mixture's model."""
    a = _crossing(model, 0.0, np.pi, 0.95)
    b = _crossing(model, a, np.pi, 0.05)
    return a + (b - a) * (np.arange(P) + 0.5) / P


def with_probes(y, init, sal, model, P):
    """Appends P probe rows with saliency 0 to every mixture; model = the oracle's model of these
    mixtures (dict mean (B, K, E), concentration (B, K), weight (B, K, 1)) that the final E-step
    will use.  -> y (B, N + P, E), init (B, K, N + P), saliency (B, N + P); the probes are the
    last P rows (their initialisation is 1 / K; with saliency 0 it does not matter)."""
    batch, N, E = y.shape
    K = init.shape[1]
    rows = np.empty((batch, P, E))
    for b in range(batch):
        mb = {k: np.asarray(v)[b] for k, v in model.items()}
        rows[b] = _circle(mb['mean'], probe_angles(mb, P))
    yp = np.concatenate([y, rows.astype(y.dtype)], axis=1)
    ip = np.concatenate([init, np.full((batch, K, P), 1.0 / K)], axis=2)
    sp = np.concatenate([sal, np.zeros((batch, P))], axis=1)
    return yp, ip, sp


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return d


def fit_reference(y, init, sal, iterations, cmin, cmax, **kw):
    """The oracle's model after `iterations` and its posteriors on the same rows."""
    y64 = np.asarray(y, np.float64)
    with np.errstate(all='ignore'):
        model = oe.vmfmm_fit(y64, init, iterations, saliency=sal, min_concentration=cmin,
                             max_concentration=cmax, **kw)
        aff = oe.vmfmm_predict(model, y64)
    return model, aff


@functools.lru_cache(maxsize=None)
def case(name, param, E, dtype='float64', K=2, N=N_ROWS, P=N_PROBES, seed=None):
    """The named scenario at feature count E: dict with y / init / saliency (probes appended: the
    last P rows), cmin / cmax / promise, the raw concentrations (B, K), and the oracle's
    one-iteration model and posteriors (`model`, `affiliation`).  Cached and read-only."""
    spec = dict(CASES[name])[param]
    sigma = spec['sigma'](E) if callable(spec['sigma']) else spec['sigma']
    if K > 2 and np.ndim(sigma):   # further classes take the last class's noise
        sigma = tuple(sigma) + (sigma[-1],) * (K - len(sigma))
    seed = 1000 * E + K if seed is None else seed
    if 'target' in spec:
        sigma = tune_sigma(E, K, N, sigma, seed, spec['target'])
    y, init, sal = scenario(E, K, N, sigma, seed, np.dtype(dtype))
    cmin, cmax = spec['cmin'], spec['cmax']
    raw = raw_concentration(y, init, sal)
    if P:
        first, _ = fit_reference(y, init, sal, 1, cmin, cmax)
        y, init, sal = with_probes(y, init, sal, first, P)
    model, aff = fit_reference(y, init, sal, 1, cmin, cmax)
    return _freeze(dict(name=name, param=param, E=E, K=K, N=N, P=P, y=y, init=init, saliency=sal,
                        cmin=cmin, cmax=cmax, promise=spec['promise'], raw=raw, model=model,
                        affiliation=aff))


def edge_rows(E=4):
    """Rows +-e_j with dyadic affiliations (16 identical mixtures of 8 rows, K = 2, no saliency):
    class 1 sees e_0 and -e_0 with 1/2 each and e_2, -e_2 with 1/4 each -- its resultant is
    exactly 0, nothing rounds -- class 0 the rest (resultant 4 e_1, class sum 6.5).
    -> y (16, 8, E) float64, init (16, 2, 8)."""
    eye = np.eye(E)
    rows = np.stack([eye[0], -eye[0], eye[1], eye[1], eye[2], -eye[2], eye[1], eye[1]])
    g1 = np.array([0.5, 0.5, 0.0, 0.0, 0.25, 0.25, 0.0, 0.0])
    y = np.tile(rows, (B, 1, 1))
    init = np.tile(np.stack([1.0 - g1, g1]), (B, 1, 1))
    return y, init
