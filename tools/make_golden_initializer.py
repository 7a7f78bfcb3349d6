"""Write the initializer fixtures tests/golden/initializer_*.npz from the live, unmodified
reference (through oracle.refshim; needs the reference tree).  Deterministic.

    python tools/make_golden_initializer.py

initializer_deflation_<F>_<T>_<D>_<K>.npz   deflationSeed of the reference on
        tests/oracle_initializer.synth_case(F, T, D, K, seed) widened to complex128, for both
        `permutation_free` values: posterior_pf0 / posterior_pf1 (K, F, T) float64 and the call
        parameters (F, T, D, K, seed, neighbors).  The input is regenerated from the seed.
initializer_iid.npz   the doctest calls of iid.py / deterministic.py under np.random.seed(0):
        <function>_pf0 / _pf1 for the four i.i.d. initialisers on np.ones([4, 5, 3]), K = 2, and
        the three flag() doctest arrays.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

# (F, T, D, K, seed, neighbors)
CASES = [(257, 64, 4, 3, 21, 5), (257, 40, 8, 4, 22, 3), (513, 48, 2, 2, 23, 5),
         (257, 96, 6, 3, 24, 5)]


def main():
    from oracle import refshim
    refshim.load()
    from pb_bss.initializer import deflation, deterministic, iid
    import oracle_initializer as oi
    os.makedirs(GOLDEN, exist_ok=True)
    for F, T, D, K, seed, nb in CASES:
        Y = oi.synth_case(F, T, D, K, seed).astype(np.complex128)
        arrays = dict(F=F, T=T, D=D, K=K, seed=seed, neighbors=nb)
        for pf in (0, 1):
            arrays[f'posterior_pf{pf}'] = np.asarray(
                deflation.deflationSeed(Y, K, permutation_free=bool(pf), neighbors=nb))
        path = os.path.join(GOLDEN, f'initializer_deflation_{F}_{T}_{D}_{K}.npz')
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path))
    arrays = {}
    ones = np.ones([4, 5, 3])
    for name in iid.__all__:
        np.random.seed(0)
        arrays[f'{name}_pf0'] = np.array(getattr(iid, name)(ones, 2))
        arrays[f'{name}_pf1'] = np.array(getattr(iid, name)(ones, 2, permutation_free=True))
    arrays['flag_4_2'] = np.array(deterministic.flag(ones, 2, permutation_free=True))
    arrays['flag_1_2_min'] = np.array(
        deterministic.flag(np.ones([1, 5, 3]), 2, minimum=0.1, permutation_free=True))
    arrays['flag_1_4_min'] = np.array(
        deterministic.flag(np.ones([1, 5, 3]), 4, minimum=0.1, permutation_free=True))
    path = os.path.join(GOLDEN, 'initializer_iid.npz')
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
