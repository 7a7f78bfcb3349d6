"""Inputs with a prescribed spectrum for the complex-Watson M-step, and the float64 trajectory
of the oracle on them (NumPy float64 only).

The device M-step keeps ONE eigenpair per class and, from the second EM iteration of a launch on,
takes it from a shifted inverse iteration started at the previous mode (csrc/wave_la.hpp:
wave_dominant_eigenpair) instead of a Jacobi decomposition.  What that shortcut has to survive is
a property of the class covariances -- the gap between the two leading eigenvalues, a mode that
jumps between two iterations, an isotropic or a rank-one class -- so the inputs here are built
from their spectrum: `block` gives unit-norm frames with an exact covariance, and with an initial
affiliation that is constant within a block every first class covariance is an exact convex
combination of block covariances.  Everything a scenario promises about the LATER iterations is
computed from `trajectory` (the loop of oracle/cwmm.py:cwmm_fit), never assumed.

Layout as in oracle/cwmm.py: Y (F, T, D), init (F, K, T).
"""
import numpy as np

from oracle import cwmm as ow

__all__ = ['block', 'unitary', 'flat_spectrum', 'class_covariance', 'trajectory',
           'covariance_after', 'leading_cluster', 'outside_cluster', 'rayleigh', 'overlap',
           'spline_slope', 'near_degenerate', 'mode_jump', 'isotropic', 'rank_one',
           'empty_class', 'self_spread', 'NEAR_DEGENERATE_D', 'MODE_JUMP_D', 'ALL_D', 'DROPPED',
           'SCENARIOS', 'GAPS', 'SHARES', 'PARITY_NEAR_DEGENERATE', 'PARITY_MODE_JUMP']

ALL_D = (2, 3, 4, 5, 6, 7, 8)
SCENARIOS = ('near_degenerate', 'mode_jump', 'isotropic', 'rank_one', 'empty_class')
# (scenario, D) pairs that cannot meet their promises, with the reason (at most one in ten of
# the 5 scenarios x 7 sensor counts; tests/test_watson_spectra_oracle.py checks the share):
DROPPED = {
    ('near_degenerate', 2): 'two leading eigenvalues fill a 2 x 2 covariance: the class is then '
                            'near-isotropic, there is no "rest" to be separated from, and any '
                            'share of a distinct second class sets the gap instead of g',
    ('near_degenerate', 3): '(0.4, 0.4 - g, 0.2 + g) is too close to isotropic (1/3): the class '
                            'loses its concentration (0.7 -> 0.04 in three iterations) and the '
                            'distance of the pair to the third eigenvalue falls below 0.05 at '
                            'iteration 1 (0.040) and to 0.005 at iteration 2',
    ('mode_jump', 2): 'the jump needs a third direction: with D = 2 the two leading eigenvalues '
                      'of the B block (0.30, 0.36) cannot have trace 1, and with (0.4, 0.6) only '
                      'share = 0.2 jumps at all',
}
NEAR_DEGENERATE_D = tuple(d for d in ALL_D if ('near_degenerate', d) not in DROPPED)
MODE_JUMP_D = tuple(d for d in ALL_D if ('mode_jump', d) not in DROPPED)
GAPS = (1e-1, 1e-3, 1e-5, 1e-6, 1e-9, 0.0)
SHARES = (0.2, 0.3, 0.4, 0.5)
# What a comparison of a whole 4-iteration trajectory with the oracle presupposes: that the
# oracle's own result does not move by more than 1e-9 (two orders below the 1e-7 it is compared
# at) when the rounding of its arithmetic changes (`self_spread`).  EM amplifies a rotation of the
# mode inside a near-degenerate plane by about kappa lam_0 lam_1 a (1 - a) / gap per iteration (a:
# the class's posterior on its own frames), so at g = 1e-5 this only holds where the posteriors
# are saturated -- D = 7, 8; measured at D = 4, 5, 6: 8e-4, 3e-5, 6e-8..1e-7.
PARITY_NEAR_DEGENERATE = tuple((g, D) for g in (1e-1, 1e-3) for D in (4, 6, 8)) + (
    (1e-5, 7), (1e-5, 8))
PARITY_MODE_JUMP = tuple(sorted({(0.3, D) for D in MODE_JUMP_D} |
                                {(s, D) for s in SHARES for D in (3, 6, 8)}))


def unitary(D, seed):
    """A Haar-like D x D unitary (QR of a complex Gaussian matrix)."""
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D)))
    return q * (np.diagonal(r) / np.abs(np.diagonal(r)))


def flat_spectrum(lead, D):
    """`lead` followed by D - len(lead) equal eigenvalues that bring the trace to 1."""
    lead = np.asarray(lead, np.float64)
    n = D - len(lead)
    assert n >= 0, (lead, D)
    if n == 0:
        assert abs(lead.sum() - 1) < 1e-15, lead
        return lead.copy()
    rest = (1.0 - lead.sum()) / n
    assert rest >= 0, (lead, D)
    return np.concatenate([lead, np.full(n, rest)])


def block(U, lam, T):
    """T unit-norm frames (T, D) whose mean outer product is exactly U diag(lam) U^H:
    y_t = U diag(sqrt(lam)) f_t with f_t[d] = exp(2 pi i d t / T) -- |f_t[d]| = 1 gives
    |y_t|^2 = sum(lam) = 1, and mean_t f_t[d] conj(f_t[e]) = [d == e] for |d - e| < T."""
    U = np.asarray(U, np.complex128)
    lam = np.asarray(lam, np.float64)
    D = U.shape[0]
    assert T >= D and lam.shape == (D,) and (lam >= 0).all(), (T, D, lam)
    assert abs(lam.sum() - 1) < 1e-14, lam.sum()
    f = np.exp(2j * np.pi * np.outer(np.arange(T), np.arange(D)) / T)  # (T, D)
    return (f * np.sqrt(lam)) @ U.T


def class_covariance(Y, aff):
    """Weighted class covariances (F, K, D, D) of the unit-normalised frames: the first two lines
    of oracle.cwmm.watson_m_step, kept so that the spectrum can be looked at."""
    y = ow.normalize_observation(np.asarray(Y, np.complex128))
    cov = np.einsum('fkn,fnd,fnD->fkdD', aff, y, y.conj())
    return cov / aff.sum(-1)[..., None, None]


def trajectory(Y, init, n, weight_constant_axis=(-1,)):
    """The loop of oracle.cwmm.cwmm_fit for n iterations -> one dict per iteration with the
    affiliation the M-step saw, the model (weight, mode, concentration) it produced, the class
    covariances and all their eigenvalues (ascending)."""
    Y = np.asarray(Y, np.complex128)
    y = ow.normalize_observation(Y)
    spline = ow.make_spline(Y.shape[-1])
    sal = np.ones_like(init[..., 0, :])
    aff, model, out = np.asarray(init, np.float64), None, []
    for _ in range(n):
        if model is not None:
            aff = ow.cwmm_predict(model, y, normalized=True)
        weight = ow.estimate_mixture_weight(aff, sal, weight_constant_axis)
        mode, conc = ow.watson_m_step(y[..., None, :, :], aff * sal[..., None, :], spline)
        model = dict(weight=weight, mode=mode, concentration=conc)
        cov = class_covariance(Y, aff)
        out.append(dict(model, affiliation=aff, covariance=cov,
                        eigenvalues=np.linalg.eigvalsh(cov)))
    return out


def covariance_after(model, Y):
    """Class covariances (F, K, D, D) the M-step that FOLLOWS `model` works on: the oracle E-step
    (oracle.cwmm.cwmm_predict) of model = dict(mode, concentration, weight (F, K, 1)), then the
    weighted covariances in float64.  A device model passes through the same function."""
    Y = np.asarray(Y, np.complex128)
    return class_covariance(Y, ow.cwmm_predict(model, Y))


def leading_cluster(cov, width):
    """-> (eigenvalues ascending, eigenvectors, n, sep): the n leading eigenvalues lie within
    `width` of the largest, `sep` is the distance from the smallest of them to the next one
    (inf when the cluster is everything)."""
    val, vec = np.linalg.eigh(cov)
    n = int((val >= val[-1] - width).sum())
    sep = np.inf if n == len(val) else float(val[-n] - val[-n - 1])
    return val, vec, n, sep


def outside_cluster(m, vec, n):
    """Norm of the component of the unit vector m outside the span of the n leading
    eigenvectors (computed from the complement's coefficients, not as 1 - inside)."""
    m = m / np.linalg.norm(m)
    D = vec.shape[0]
    return float(np.linalg.norm(vec[:, :D - n].conj().T @ m))


def rayleigh(m, cov):
    m = m / np.linalg.norm(m)
    return float((m.conj() @ cov @ m).real)


def overlap(a, b):
    """|a^H b| of the normalised vectors, along the last axis."""
    return np.abs(np.einsum('...d,...d->...', np.conj(a), b)) / (
        np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def spline_slope(spline, x, h=1e-6):
    """Finite-difference slope of the oracle's eigenvalue -> concentration spline at x."""
    return float(abs(spline(x + h) - spline(x - h)) / (2 * h))


def _two_block(blocks, shares, F, T, D, seed):
    """F bins of two blocks of T / 2 frames each; blocks(U) -> the two (T/2, D) arrays on the
    bin's own random basis; shares = class 0's initial affiliation on the two blocks."""
    assert T % 2 == 0
    h = T // 2
    Y = np.empty((F, T, D), np.complex128)
    init = np.empty((F, 2, T))
    for f in range(F):
        a, b = blocks(unitary(D, seed + 101 * f), h)
        Y[f, :h], Y[f, h:] = a, b
        init[f, 0, :h], init[f, 0, h:] = shares
    init[:, 1] = 1.0 - init[:, 0]
    return Y, init


def _promises(Y, init, n, cls=0):
    """Per iteration, over all bins, of class `cls`: smallest / largest gap between the two
    leading eigenvalues, smallest distance from the second eigenvalue to the third (inf for
    D = 2), concentration range, and the smallest overlap of consecutive modes."""
    tr = trajectory(Y, init, n)
    out = []
    for i, s in enumerate(tr):
        ev = s['eigenvalues'][:, cls]
        gap = ev[:, -1] - ev[:, -2]
        sep = ev[:, -2] - ev[:, -3] if ev.shape[-1] > 2 else np.full(len(ev), np.inf)
        conc = s['concentration'][:, cls]
        ov = overlap(tr[i - 1]['mode'][:, cls], s['mode'][:, cls]) if i else np.ones(len(ev))
        out.append(dict(gap_min=float(gap.min()), gap_max=float(gap.max()),
                        sep_min=float(sep.min()), conc_min=float(conc.min()),
                        conc_max=float(conc.max()), overlap_min=float(ov.min()),
                        overlap_max=float(ov.max())))
    return tr, out


def near_degenerate(g, D=6, F=3, T=192, seed=0, iterations=4):
    """Class 0 mostly (0.9 / 0.1) sees a block with leading eigenvalues (0.4, 0.4 - g), the rest
    flat; class 1 a block with (0.7, 0.1, flat) on the reversed basis (D >= 4: the two leading
    directions of class 0 then see equal eigenvalues of the class-1 block, and the top gap of
    class 0's first covariance is exactly 0.9 g).
    -> Y, init, props(trajectory=..., per_iteration=[...])."""
    assert ('near_degenerate', D) not in DROPPED, DROPPED['near_degenerate', D]

    def blocks(U, h):
        return (block(U, flat_spectrum([0.4, 0.4 - g], D), h),
                block(U[:, ::-1], flat_spectrum([0.7, 0.1], D), h))
    Y, init = _two_block(blocks, (0.9, 0.1), F, T, D, seed)
    tr, per = _promises(Y, init, iterations)
    return Y, init, dict(trajectory=tr, per_iteration=per, g=g)


def mode_jump(share, D=6, F=3, T=192, seed=0, iterations=4):
    """Block A has (0.9, 0.02, flat) on the basis U, block B (0.30, 0.36, flat) on the same U;
    class 0 starts with `share` on A and 0.95 on B.  Its first covariance has u_0 on top; after
    an E-step it keeps B and u_1 leads: the warm start of that iteration is an exact eigenvector
    of the new covariance that belongs to its SECOND eigenvalue.  D = 3: B is (0.30, 0.45, 0.25)
    -- with 0.36 the one remaining eigenvalue, 0.34, would sit 0.02 below the leading one.
    props['jump_at'] is the iteration of the jump (1 at D = 6; 1 or 2 elsewhere), the first at
    which the overlap of consecutive class-0 modes is below 0.5 in every bin."""
    assert ('mode_jump', D) not in DROPPED, DROPPED['mode_jump', D]
    lead_b = [0.30, 0.45] if D == 3 else [0.30, 0.36]

    def blocks(U, h):
        return (block(U, flat_spectrum([0.9, 0.02], D), h),
                block(U, flat_spectrum(lead_b, D), h))
    Y, init = _two_block(blocks, (share, 0.95), F, T, D, seed)
    tr, per = _promises(Y, init, iterations)
    jumps = [i for i, q in enumerate(per) if q['overlap_max'] < 0.5]
    return Y, init, dict(trajectory=tr, per_iteration=per, share=share,
                         jump_at=jumps[0] if jumps else None)


def _one_class(lams, D, T, seed, iterations):
    F = len(lams)
    Y = np.stack([block(unitary(D, seed + 101 * f), lams[f], T) for f in range(F)])
    init = np.ones((F, 1, T))
    tr, per = _promises(Y, init, iterations)
    return Y, init, dict(trajectory=tr, per_iteration=per)


def isotropic(D=6, F=3, T=192, seed=0, iterations=3):
    """One class (K = 1: the affiliation is 1 at every iteration) whose block has lam = 1 / D
    throughout: every vector is an eigenvector, the covariance is the same at every iteration."""
    return _one_class([np.full(D, 1.0 / D)] * F, D, T, seed, iterations)


def rank_one(D=6, F=4, T=192, seed=0, iterations=3):
    """One class (K = 1) whose block is rank one: even bins lam = (1 - (D-1) 1e-12, 1e-12, ...),
    odd bins exactly (1, 0, ...).  The eigenvalue is above the spline's range, the concentration
    sits at max_concentration, and sigma I - C is nearly singular in one direction."""
    soft = np.concatenate([[1.0 - (D - 1) * 1e-12], np.full(D - 1, 1e-12)])
    hard = np.concatenate([[1.0], np.zeros(D - 1)])
    return _one_class([soft if f % 2 == 0 else hard for f in range(F)], D, T, seed, iterations)


def empty_class(D=6, F=4, T=192, seed=0, empty_bin=1, iterations=3):
    """Two classes on blocks with (0.7, flat) on a basis and on its reverse (0.9 / 0.1), and in
    bin `empty_bin` class 1 of `init` exactly zero: that class's covariance is 0 / 0.
    -> Y, init, props(empty_bin, keep = the other bins, trajectory of the other bins)."""
    def blocks(U, h):
        return (block(U, flat_spectrum([0.7], D), h),
                block(U[:, ::-1], flat_spectrum([0.7], D), h))
    Y, init = _two_block(blocks, (0.9, 0.1), F, T, D, seed)
    init[empty_bin, 0] = 1.0
    init[empty_bin, 1] = 0.0
    keep = [f for f in range(F) if f != empty_bin]
    tr, per = _promises(Y[keep], init[keep], iterations)
    return Y, init, dict(empty_bin=empty_bin, keep=keep, trajectory=tr, per_iteration=per)


def self_spread(Y, init, n, weight_constant_axis=(-1,)):
    """The oracle's own error on this input: the largest change of the final affiliations and of
    the final concentrations (relative to the largest) between the n-iteration trajectory of Y and
    that of Y with every frame multiplied by a phase of its own -- the same model in exact
    arithmetic (y y^H is unchanged), other roundings."""
    rng = np.random.default_rng(12345)
    Y = np.asarray(Y, np.complex128)
    Z = Y * np.exp(2j * np.pi * rng.uniform(size=Y.shape[:2]))[..., None]
    a = trajectory(Y, init, n, weight_constant_axis)[-1]
    b = trajectory(Z, init, n, weight_constant_axis)[-1]
    aff = np.abs(ow.cwmm_predict(a, Y) - ow.cwmm_predict(b, Z)).max()
    conc = np.abs(a['concentration'] - b['concentration']).max() / a['concentration'].max()
    return float(aff), float(conc)
