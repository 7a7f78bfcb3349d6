#!/usr/bin/env python3
"""Class-count sweep of the real-embedding mixtures: time per EM iteration of the vMF and the
spherical-Gaussian mixture for K = 8 (csrc/embed.hip) against K = 9, 16, 32, 64
(csrc/embed_wide.hip) on the same N and E, and of the joint fit for K = 8, 12, 19.

    python tools/bench_embed_wide.py [--out profiles/embed_wide_classes.json] [--no-joint]

Device time from HIP events around the enqueued loop (pbbss_set_timing) over ITER iterations,
after one warm-up fit per shape; the median of REPS repeats.  Per (row x class) cost, the share of
the FP64 matrix peak (2 * 2 N E K flop per iteration: E-step and M-step contractions) and of the
HBM bandwidth (one read of y per iteration) are derived from the shapes; the joint rows count
the spatial half too (see joint())."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pb_bss_amd import _lib, engine

ITER, REPS = 50, 7
PEAK_FP64_MATRIX = 78.6e12  # flop/s, MI355X FP64 matrix
PEAK_HBM = 8.0e12           # bytes/s


def labelled(N, E, K, seed):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((K, E)) * 1.5
    lab = rng.integers(K, size=N)
    y = (mu[lab] + 0.7 * rng.standard_normal((N, E))).astype(np.float32)
    init = rng.uniform(size=(K, N)) + 2.0 * (np.arange(K)[:, None] == lab[None, :])
    return y, init / init.sum(0)


def timed(fn):
    fn()  # warm-up: code objects, workspace growth
    ms = []
    for _ in range(REPS):
        fn()
        torch.cuda.synchronize()
        ms.append(engine.last_kernel_ms())
    return statistics.median(ms), min(ms), max(ms)


def mixtures():
    rows = []
    for N in (30000, 256500):
        for K in (8, 9, 16, 32, 64):
            y, init = labelled(N, 40, K, N + K)
            yd = _lib.to_device(y).reshape(1, N, 40)
            g0 = _lib.to_device(init).reshape(1, K, N).contiguous()
            for name, fit in (('vmfmm', engine.vmfmm_fit), ('gmm_spherical', engine.gmm_fit)):
                med, lo, hi = timed(lambda: fit(yd, K, gamma0=g0, iterations=ITER))
                us = med / ITER * 1e3
                rows.append(dict(
                    model=name, N=N, E=40, K=K, path='embed.hip' if K <= 8 else 'embed_wide.hip',
                    us_per_iteration=round(us, 2), us_min=round(lo / ITER * 1e3, 2),
                    us_max=round(hi / ITER * 1e3, 2),
                    ps_per_row_class=round(us * 1e6 / (N * K), 3),
                    fp64_matrix_peak_fraction=round(4.0 * N * 40 * K / (us * 1e-6) / PEAK_FP64_MATRIX, 4),
                    hbm_peak_fraction=round(N * 40 * 4 / (us * 1e-6) / PEAK_HBM, 4)))
                print(rows[-1], flush=True)
    # beyond E = 60 the row block shrinks to 32 and 16 rows (fewer wavefronts per workgroup work on
    # the contractions) and column tiles are split over gridDim.z: the cost of that, at K = 16
    for E in (40, 64, 128, 256):
        N, K = 100000, 16
        rng = np.random.default_rng(E)
        yd = _lib.to_device(rng.standard_normal((N, E)).astype(np.float32)).reshape(1, N, E)
        g = rng.uniform(size=(K, N))
        g0 = _lib.to_device(g / g.sum(0)).reshape(1, K, N).contiguous()
        med, lo, hi = timed(lambda: engine.gmm_fit(yd, K, gamma0=g0, iterations=ITER))
        us = med / ITER * 1e3
        rows.append(dict(model='gmm_spherical', N=N, E=E, K=K, path='embed_wide.hip',
                         us_per_iteration=round(us, 2), us_min=round(lo / ITER * 1e3, 2),
                         us_max=round(hi / ITER * 1e3, 2),
                         ps_per_row_class_feature=round(us * 1e6 / (N * K * E), 4),
                         fp64_matrix_peak_fraction=round(4.0 * N * E * K / (us * 1e-6) / PEAK_FP64_MATRIX, 4),
                         hbm_peak_fraction=round(N * E * 4 / (us * 1e-6) / PEAK_HBM, 4)))
        print(rows[-1], flush=True)
    return rows


def joint():
    from oracle import synth
    rows = []
    F, T, D, E = 513, 500, 8, 40
    for K in (8, 12, 19):
        Y, e, init = synth.make_joint(F, T, D, K, E, seed=K)
        yd, ed, gd = _lib.to_device(Y), _lib.to_device(e), _lib.to_device(init)
        it = 10
        med, lo, hi = timed(lambda: engine.joint_fit(yd, ed, K, _lib.EMBED_GAUSS_SPHERICAL,
                                                     gamma0=gd, iterations=it))
        # what one iteration needs by the shapes: both spectral contractions (4 N E K) and, per
        # point and class, the spatial quadratic form and the covariance update (8 D^2 each);
        # bytes: embedding and observation read once, posteriors (F, K, T) written and read once
        N, sec = F * T, med / it * 1e-3
        flop = 4.0 * N * E * K + 16.0 * N * K * D * D
        byts = N * E * 4 + N * D * 8 + 2 * 8 * N * K
        rows.append(dict(model='gcacgmm', F=F, T=T, D=D, E=E, K=K,
                         us_per_iteration=round(med / it * 1e3, 1),
                         us_min=round(lo / it * 1e3, 1), us_max=round(hi / it * 1e3, 1),
                         fp64_peak_fraction=round(flop / sec / PEAK_FP64_MATRIX, 4),
                         hbm_peak_fraction=round(byts / sec / PEAK_HBM, 4)))
        print(rows[-1], flush=True)
    return rows


def main():
    engine.set_timing(True)
    out = dict(device=torch.cuda.get_device_name(0), iterations=ITER, repeats=REPS,
               mixtures=mixtures())
    if '--no-joint' not in sys.argv:
        out['joint'] = joint()
    if '--out' in sys.argv:
        path = sys.argv[sys.argv.index('--out') + 1]
        with open(path, 'w') as f:
            json.dump(out, f, indent=1)
        print('wrote', path)


if __name__ == '__main__':
    main()
