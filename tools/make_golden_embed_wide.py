#!/usr/bin/env python3
"""Record tests/golden/embed_wide_*.npz from the UNMODIFIED reference (imported through
oracle/refshim.py): mixtures with more than eight classes -- inputs, initialisation and the
reference's outputs only.

    python tools/make_golden_embed_wide.py          (needs the reference tree)

    vMF mixture     VMFMMTrainer.fit                              K = 12, N = 600, E = 10, 5 iterations, saliency
    spherical GMM   GMMTrainer.fit(covariance_type='spherical')   same
    joint           GCACGMMTrainer.fit                            (F, T, D, K, E) = (6, 120, 5, 10, 8), 4 iterations
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def mixture_inputs(N=600, E=10, K=12, seed=2024):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((K, E)) * 1.5
    lab = rng.integers(K, size=N)
    y = (mu[lab] + 0.6 * rng.standard_normal((N, E))).astype(np.float32).astype(np.float64)
    init = rng.uniform(size=(K, N)) + 2.0 * (np.arange(K)[:, None] == lab[None, :])
    init /= init.sum(0)
    sal = rng.uniform(0.1, 1.0, size=N)
    return y, init, sal


def joint_inputs(F=6, T=120, D=5, K=10, E=8, seed=2025):
    from oracle import synth
    Y, e, init = synth.make_joint(F, T, D, K, E, seed=seed)
    return Y.astype(np.complex128), e.astype(np.float64), init


def main():
    from oracle import refshim
    refshim.load()
    from pb_bss.distribution import GCACGMMTrainer, GMMTrainer, VMFMMTrainer
    y, init, sal = mixture_inputs()
    it = 5
    m = VMFMMTrainer().fit(y, initialization=init, iterations=it, saliency=sal)
    np.savez_compressed(os.path.join(GOLDEN, 'embed_wide_vmfmm_n600_e10_k12.npz'), y=y, init=init,
                        saliency=sal, iterations=it, mean=m.vmf.mean, scale=m.vmf.concentration,
                        weight=m.weight, affiliation=m.predict(y))
    g = GMMTrainer().fit(y, initialization=init, iterations=it, saliency=sal,
                         covariance_type='spherical')
    np.savez_compressed(os.path.join(GOLDEN, 'embed_wide_gmm_n600_e10_k12.npz'), y=y, init=init,
                        saliency=sal, iterations=it, mean=g.gaussian.mean,
                        scale=g.gaussian.covariance, weight=g.weight, affiliation=g.predict(y))
    Y, e, jinit = joint_inputs()
    j = GCACGMMTrainer().fit(Y, e, initialization=jinit, iterations=4)
    np.savez_compressed(os.path.join(GOLDEN, 'embed_wide_gcacgmm_f6_t120_d5_k10_e8.npz'),
                        Y=Y.astype(np.complex64), embedding=e.astype(np.float32), init=jinit,
                        iterations=4, mean=j.gaussian.mean, covariance=j.gaussian.covariance,
                        weight=np.asarray(j.weight), affiliation=j.predict(Y, e))
    for name in sorted(os.listdir(GOLDEN)):
        if name.startswith('embed_wide_'):
            print(name, os.path.getsize(os.path.join(GOLDEN, name)), 'bytes')


if __name__ == '__main__':
    main()
