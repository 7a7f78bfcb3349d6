"""Write the complex-Bingham fixtures tests/golden/cbmm_*.npz from the live reference (through
oracle.refshim; needs the reference tree).  Deterministic (fixed seeds).

    python tools/make_golden_cbmm.py

cbmm_spectra.npz   find_eigenvalues_v3 on 48 scatter spectra, D = 2..6: the doctest vectors,
                   Dirichlet spectra, near-duplicate and ill-conditioned ones (smallest eigenvalue
                   1e-9 .. 1e-5), max_concentration = inf and 500; per D: s_D<d>, maxc_D<d>,
                   lam_D<d>
cbmm_norm.npz      ComplexBingham.norm() of eigenvalue vectors (the doctest vectors included);
                   lam_D<d>, norm_D<d>
cbmm_fit_<name>.npz  short CBMMTrainer.fit runs from a fixed initialisation and their predict():
                   y, init, iterations, kwargs (repr), weight, eigvec, eigval, affiliation
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

DOCTEST = [
    ([0.9, 0.1], np.inf), ([0.5, 0.5], np.inf), ([0.9, 0.06, 0.04], np.inf),
    ([0.9, 0.05, 0.05], np.inf), ([0.9, 0.0666666667, 0.0333333333], np.inf),
    ([0.9, 0.06, 0.03, 0.006, 0.003, 0.001], np.inf),
    ([5.15996555e-04, 6.28805516e-04, 1.37554184e-03, 1.53621463e-02, 3.74437619e-02,
      9.44673748e-01], np.inf),
    ([5.15996555e-04, 6.28805516e-04, 1.37554184e-03, 1.53621463e-02, 3.74437619e-02,
      9.44673748e-01], 500.0),
]

FITS = {
    'cbmm_fit_d3_k2': dict(F=4, T=120, D=3, K=2, seed=1, kwargs={}),
    'cbmm_fit_d4_k3': dict(F=4, T=120, D=4, K=3, seed=2, kwargs={}),
    'cbmm_fit_d6_k3_saliency': dict(F=3, T=150, D=6, K=3, seed=3, kwargs={}, saliency=True),
    'cbmm_fit_d4_k2_uniform': dict(F=4, T=120, D=4, K=2, seed=4,
                                   kwargs={'weight_constant_axis': -2}),
}


def spectra():
    rng = np.random.default_rng(0)
    out = {}
    for s, maxc in DOCTEST:
        out.setdefault(len(s), []).append((np.asarray(s, dtype=np.float64), maxc))
    for D in range(2, 7):
        for i in range(8):
            s = np.sort(rng.dirichlet(np.ones(D) * rng.uniform(0.3, 3.0)))
            if i == 5:  # near-duplicate pair
                s[1] = s[0] * (1 + 1e-7)
            if i in (6, 7):  # one small, well separated eigenvalue
                s[0] = 10.0 ** (-9 if i == 6 else -5)
            s = np.sort(s / s.sum())
            out.setdefault(D, []).append((s, np.inf if i % 2 else 500.0))
    return out


def mixture(F, T, D, K, seed):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((F, T, D)) + 1j * rng.standard_normal((F, T, D))
    dirs = rng.standard_normal((F, K, D)) + 1j * rng.standard_normal((F, K, D))
    lab = rng.integers(0, K, size=(F, T))
    y += 3 * np.take_along_axis(dirs, lab[..., None], axis=1) * rng.standard_normal((F, T, 1))
    init = rng.uniform(size=(F, K, T))
    init /= init.sum(1, keepdims=True)
    return y, init


def main():
    from oracle import refshim
    refshim.load()
    from pb_bss.distribution.cbmm import CBMMTrainer
    from pb_bss.distribution.complex_bingham import ComplexBingham, ComplexBinghamTrainer
    os.makedirs(GOLDEN, exist_ok=True)
    arrays = {}
    for D, items in spectra().items():
        s = np.stack([x for x, _ in items])
        maxc = np.array([m for _, m in items])
        lam = np.stack([ComplexBinghamTrainer.find_eigenvalues_v3(x, max_concentration=m)
                        for x, m in items])
        arrays.update({f's_D{D}': s, f'maxc_D{D}': maxc, f'lam_D{D}': lam})
    np.savez_compressed(os.path.join(GOLDEN, 'cbmm_spectra.npz'), **arrays)
    rng = np.random.default_rng(1)
    norms = {}
    for D in range(2, 7):
        lam = -np.sort(np.abs(rng.standard_normal((6, D))) * 10.0 ** rng.uniform(0, 2, (6, 1)), -1)
        lam -= lam.max(-1, keepdims=True)
        if D == 3:
            lam = np.concatenate([lam, [[0.8, 0.92679492, 1.27320508], [1, 0.1, 0.1],
                                        [1, 0.1, 0.0]]])
        if D == 6:
            lam = np.concatenate([lam, [[5.15996555e-04, 6.28805516e-04, 1.37554184e-03,
                                         1.53621463e-02, 3.74437619e-02, 9.44673748e-01],
                                        [-10.00000004, -10.00000003, -10.00000002, -10.00000001,
                                         -10.0, 0.0]]])
        norms[f'lam_D{D}'] = lam
        norms[f'norm_D{D}'] = np.array([ComplexBingham(None, x).norm() for x in lam])
    np.savez_compressed(os.path.join(GOLDEN, 'cbmm_norm.npz'), **norms)
    for name, c in FITS.items():
        y, init = mixture(c['F'], c['T'], c['D'], c['K'], c['seed'])
        kw = dict(c['kwargs'])
        sal = None
        if c.get('saliency'):
            sal = np.random.default_rng(c['seed']).uniform(size=(c['F'], c['T']))
            kw['saliency'] = sal
        model = CBMMTrainer().fit(y, initialization=init, iterations=10, **kw)
        aff = model.predict(y)
        np.savez_compressed(
            os.path.join(GOLDEN, name + '.npz'), y=y, init=init, iterations=10,
            kwargs=repr(c['kwargs']), saliency=np.zeros(0) if sal is None else sal,
            weight=np.asarray(model.weight, dtype=np.float64),
            eigvec=model.complex_bingham.covariance_eigenvectors,
            eigval=model.complex_bingham.covariance_eigenvalues, affiliation=aff)
    for f in sorted(os.listdir(GOLDEN)):
        if f.startswith('cbmm_'):
            print(f, os.path.getsize(os.path.join(GOLDEN, f)))


if __name__ == '__main__':
    main()
