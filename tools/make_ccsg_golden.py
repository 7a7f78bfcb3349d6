"""Write the complex circular-symmetric Gaussian fixtures tests/golden/ccsg_*.npz from the live,
unmodified reference (through oracle.refshim; needs the reference tree).  Deterministic.

    python tools/make_ccsg_golden.py

The inputs are regenerated from seeds by tests/oracle_ccsg.py (`case`, widened to complex128 /
float64: the comparison target of a complex64 run is the result on the widened values); the
files hold the reference's outputs only.

ccsg_reference.npz   for every case of oracle_ccsg.FIXTURE_CASES: `<key>/cov` the trainer's
        covariance (B, K, D, D) and `<key>/lp` the log-pdf (B, K, N) of the case's own
        well-conditioned covariances; `sample` the draws of
        ComplexCircularSymmetricGaussian(sample_covariance()).sample(SAMPLE_SIZE) under
        np.random.seed(SAMPLE_SEED).
ccsg_names.txt       the names that pb_bss/distribution/__init__.py imports.
"""
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def imported_names(path):
    """Every name an `import` statement of the module at `path` binds."""
    with open(path) as f:
        tree = ast.parse(f.read())
    names = []
    for node in tree.body:
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            names += [(a.asname or a.name).split('.')[0] for a in node.names]
    return sorted(set(names))


def main():
    from oracle import refshim
    refshim.load()
    from pb_bss.distribution.complex_circular_symmetric_gaussian import (
        ComplexCircularSymmetricGaussian, ComplexCircularSymmetricGaussianTrainer)
    import oracle_ccsg as oc
    os.makedirs(GOLDEN, exist_ok=True)
    arrays = {}
    for D, N, K, B, y_dtype, sal_dtype in oc.FIXTURE_CASES:
        y, s, cov = oc.case(D, N, K, B, y_dtype, sal_dtype)
        y = y.astype(np.complex128)
        key = oc.case_key(D, N, K, B, y_dtype, sal_dtype)
        trainer = ComplexCircularSymmetricGaussianTrainer()
        if s is None:
            fitted = trainer.fit(y).covariance[:, None]
        else:
            fitted = trainer.fit(y[:, None], saliency=s.astype(np.float64)).covariance
        arrays[key + '/cov'] = fitted
        arrays[key + '/lp'] = ComplexCircularSymmetricGaussian(covariance=cov).log_pdf(y[:, None])
    np.random.seed(oc.SAMPLE_SEED)
    arrays['sample'] = ComplexCircularSymmetricGaussian(
        covariance=oc.sample_covariance()).sample(oc.SAMPLE_SIZE)
    path = os.path.join(GOLDEN, 'ccsg_reference.npz')
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path))

    init = os.path.join(refshim.REFERENCE_ROOT, 'pb_bss', 'distribution', '__init__.py')
    path = os.path.join(GOLDEN, 'ccsg_names.txt')
    with open(path, 'w') as f:
        f.write('\n'.join(imported_names(init)) + '\n')
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
