"""CPU: the complex-Bingham oracle (tests/oracle_cbmm.py) against mpmath and against the live
reference, and the import surface of the new model."""
import numpy as np
import pytest

import oracle_cbmm as oc


def test_import_surface():
    from pb_bss_amd import _lib
    from pb_bss_amd.distribution import CBMM, CBMMTrainer, ComplexBingham, ComplexBinghamTrainer
    from pb_bss_amd.distribution.complex_bingham import force_hermitian, normalize_observation
    assert callable(force_hermitian) and callable(normalize_observation)
    assert CBMM and CBMMTrainer and ComplexBingham
    assert 'eignevalue_eps' in ComplexBinghamTrainer.__init__.__code__.co_varnames
    assert {'pbbss_cbmm_fit', 'pbbss_cbingham_find_eigenvalues'} <= set(_lib.EXPORTS)
    A = np.array([[1 + 2j, 3 + 5j], [7 + 11j, 13 + 17j]])
    assert np.allclose(force_hermitian(A), [[1, 5 - 3j], [5 + 3j, 13]])
    inv, srt = ComplexBingham._remove_duplicate_eigenvalues(np.array([1, 0.0, 0.0]))
    assert list(inv) == [2, 0, 1] and np.allclose(srt, [0, 1e-8, 1 + 1e-8], rtol=0, atol=1e-15)


def _mp_lne_g_h(lam):
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 60
    x = [mp.mpf(float(v)) for v in lam]
    D = len(x)

    def lne(*v):
        tab = [mp.e ** t for t in v]
        for lvl in range(1, len(v)):
            tab = [(tab[i + 1] - tab[i]) / (v[i + lvl] - v[i]) for i in range(len(v) - lvl)]
        return mp.log(tab[0])

    def at(i, t, j=None, u=None):
        v = list(x)
        v[i] = t
        if j is not None:
            v[j] = u
        return v

    g = [mp.diff(lambda t, i=i: lne(*at(i, t)), x[i]) for i in range(D)]
    H = [[None] * D for _ in range(D)]
    for i in range(D):
        H[i][i] = mp.diff(lambda t, i=i: lne(*at(i, t)), x[i], 2)
        for j in range(i + 1, D):
            H[i][j] = H[j][i] = mp.diff(lambda t, u, i=i, j=j: lne(*at(i, t, j, u)),
                                        (x[i], x[j]), (1, 1))
    return (float(lne(*x)), np.array([float(v) for v in g]),
            np.array([[float(v) for v in row] for row in H]))


@pytest.mark.parametrize('D', [2, 3, 5, 6])
def test_normaliser_vs_mpmath(D):
    """ln c, g and H of the oracle within 1e-13 of 60-digit mpmath, nodes 1e-8 .. 1e-3 apart
    included: ln e relative, every g_i relative, H_ij relative to the larger of sqrt(H_ii H_jj)
    and g_i g_j -- H = (1 + d_ij) e[lam, lam_i, lam_j] / e[lam] - g_i g_j is a difference of terms
    of size g_i g_j, which for the largest node (g ~ 1, H ~ 1e-3) is where its digits go.  H is
    only the Jacobian of the solve: its accuracy sets the convergence rate, not the solution."""
    rng = np.random.default_rng(D)
    for trial in range(3):
        lam = np.sort(-np.abs(rng.standard_normal(D)) * 10 ** rng.uniform(0, 2.5))
        if trial % 2 and D >= 3:  # nodes 1e-8 .. 1e-3 apart
            lam[1:3] = lam[1] + 10 ** rng.uniform(-8, -3) * np.arange(2)
        lam = np.sort(lam) - lam.max()
        lne, g, H = _mp_lne_g_h(lam)
        l, go, Ho = oc.grad_hess(lam[None])
        assert abs(l[0] - lne) <= 1e-13 * max(1.0, abs(lne))
        assert (np.abs(go[0] - g) <= 1e-13 * np.abs(g)).all(), np.abs(go[0] / g - 1).max()
        scale = np.maximum(np.sqrt(np.outer(np.diag(H), np.diag(H))), np.outer(g, g))
        assert (np.abs(Ho[0] - H) <= 1e-13 * scale).all(), (np.abs(Ho[0] - H) / scale).max()


def _golden(name):
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                                name + '.npz'))


def test_oracle_reproduces_reference_fixtures():
    """tests/golden/cbmm_*.npz (tools/make_golden_cbmm.py, the live reference): the oracle's
    residual is no worse than the reference's on every spectrum; ln c agrees where the
    reference's partial fractions are well conditioned (gaps >= 0.1); the short fits agree to
    the reference's own solver noise (2e-3)"""
    import ast
    g = _golden('cbmm_spectra')
    n_spec = 0
    for D in range(2, 7):
        s, maxc, lam_ref = g[f's_D{D}'], g[f'maxc_D{D}'], g[f'lam_D{D}']
        for i in range(len(s)):
            lo = oc.find_eigenvalues_v3(s[i:i + 1], max_concentration=maxc[i])
            ro = np.linalg.norm(oc.residual(s[i:i + 1], lo))
            rr = np.linalg.norm(oc.residual(s[i:i + 1], lam_ref[i:i + 1]))
            assert ro <= rr * (1 + 1e-6) + 1e-13, (D, i)
            assert (lo >= -maxc[i]).all()
            n_spec += 1
    assert n_spec == 48
    nm = _golden('cbmm_norm')
    for D in range(2, 7):
        lam, ref = nm[f'lam_D{D}'], nm[f'norm_D{D}']
        ok = np.diff(np.sort(lam, -1), axis=-1).min(-1) >= 0.1
        assert ok.sum() >= 2
        assert np.abs(np.exp(oc.log_norm(lam[ok])) / ref[ok] - 1).max() < 1e-10
    for name in ('cbmm_fit_d3_k2', 'cbmm_fit_d4_k3', 'cbmm_fit_d6_k3_saliency',
                 'cbmm_fit_d4_k2_uniform'):
        f = _golden(name)
        kw = ast.literal_eval(str(f['kwargs']))
        ref = oc.cbmm_fit(f['y'], f['init'], int(f['iterations']),
                          saliency=f['saliency'] if f['saliency'].size else None,
                          uniform=kw.get('weight_constant_axis') == -2)
        assert np.abs(oc.cbmm_predict(ref, f['y']) - f['affiliation']).max() < 2e-3
        w = ref['weight'] if kw.get('weight_constant_axis') != -2 else ref['weight'][0]
        assert np.abs(w - f['weight']).max() < 2e-3


@pytest.mark.needs_reference
def test_solver_no_worse_than_reference():
    from oracle import refshim
    refshim.load()
    from pb_bss.distribution.complex_bingham import ComplexBinghamTrainer as Ref
    rng = np.random.default_rng(4)
    for D in range(2, 7):
        for i in range(6):
            s = np.sort(rng.dirichlet(np.ones(D) * rng.uniform(0.3, 3)))
            maxc = np.inf if i % 2 else 500.0
            lr = Ref.find_eigenvalues_v3(s, max_concentration=maxc)
            lo = oc.find_eigenvalues_v3(s[None], max_concentration=maxc)[0]
            rr = np.linalg.norm(oc.residual(s[None], lr[None]))
            ro = np.linalg.norm(oc.residual(s[None], lo[None]))
            assert ro <= rr * (1 + 1e-6) + 1e-13
            assert (lo >= -maxc).all() and lo.max() <= 1e-6
            if np.isinf(maxc) and np.diff(s).min() >= 1e-3:
                assert np.abs(lo - lr).max() <= 1e-4 * max(1.0, np.abs(lr).max())


@pytest.mark.needs_reference
def test_short_fit_vs_reference():
    from oracle import refshim
    refshim.load()
    from pb_bss.distribution.cbmm import CBMMTrainer as Ref
    rng = np.random.default_rng(6)
    F, T, D, K = 3, 200, 3, 2
    y = rng.standard_normal((F, T, D)) + 1j * rng.standard_normal((F, T, D))
    init = rng.uniform(size=(F, K, T))
    init /= init.sum(1, keepdims=True)
    ref = Ref().fit(y, initialization=init, iterations=5).predict(y)
    ora = oc.cbmm_predict(oc.cbmm_fit(y, init, 5), y)
    assert np.abs(ref - ora).max() <= 2e-3
