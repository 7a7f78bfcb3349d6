"""CPU: the premises of tests/test_gpu_ccsg.py.

1. The NumPy restatement of tests/oracle_ccsg.py equals the live reference where the tree is
   present and the committed fixtures always (1e-13 relative: the same arithmetic), so it may
   serve as the GPU tests' reference where no fixture exists.
2. What the reference does at its edges (measured on the live reference; the device classes
   reproduce all of it but the last, the documented deviation).
3. The oracle's log-pdf error against its longdouble restatement, relative to max|log_pdf|, per
   conditioning case: printed under `pytest -s`, copied into the GPU file's table and docstring;
   the table must bound what is measured here by no more than a factor 4.
4. The D, N and K lists of the GPU sweep reach both sides of every instantiation boundary, every
   frame-tile / span boundary and every class-tile count of the kernels, read from
   pb_bss_amd.engine.
5. Every name the reference's distribution/__init__.py imports is an attribute of
   pb_bss_amd.distribution.
"""
import ast
import os

import numpy as np
import pytest

import oracle_ccsg as oc
from oracle import refshim

HERE = os.path.dirname(os.path.abspath(__file__))


def reference():
    refshim.load()
    from pb_bss.distribution import complex_circular_symmetric_gaussian as ref
    return ref


def rel(a, b):
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / (scale if scale else 1.0))


def widened(D, N, K, B, y_dtype, sal_dtype):
    y, s, cov = oc.case(D, N, K, B, y_dtype, sal_dtype)
    return y.astype(np.complex128), None if s is None else s.astype(np.float64), cov


# ---- 1. restatement against the live reference and the fixtures ----------------------------------
@pytest.mark.needs_reference
def test_restatement_equals_the_live_reference():
    ref = reference()
    for D in (1, 3, 8, 17):
        for N, K, B, y_dtype, sal_dtype in oc.sweep_cases(D)[:6]:
            y, s, cov = widened(D, N, K, B, y_dtype, sal_dtype)
            trainer = ref.ComplexCircularSymmetricGaussianTrainer()
            want = (trainer.fit(y).covariance[:, None] if s is None
                    else trainer.fit(y[:, None], saliency=s).covariance)
            assert rel(oc.oracle_fit(y, s), want) <= 1e-13
            want = ref.ComplexCircularSymmetricGaussian(covariance=cov).log_pdf(y[:, None])
            assert rel(oc.log_pdf(y[:, None], cov), want) <= 1e-13


def test_restatement_equals_the_fixtures():
    fx = oc.fixtures()
    assert len(oc.FIXTURE_CASES) >= 8
    for c in oc.FIXTURE_CASES:
        y, s, cov = widened(*c)
        key = oc.case_key(*c)
        assert rel(oc.oracle_fit(y, s), fx[key + '/cov']) <= 1e-13, key
        assert rel(oc.log_pdf(y[:, None], cov), fx[key + '/lp']) <= 1e-13, key


def test_extended_precision_restatement_agrees():
    for c in oc.FIXTURE_CASES[:8]:
        y, s, cov = widened(*c)
        assert rel(oc.oracle_fit(y, s, oc.fit_ext).astype(np.complex128),
                   oc.oracle_fit(y, s)) <= 1e-13
        lp, log_det = oc.log_pdf_ext(y[:, None], cov)
        assert rel(lp.astype(np.float64), oc.log_pdf(y[:, None], cov)) <= 1e-12
        np.testing.assert_allclose(log_det.astype(np.float64), np.linalg.slogdet(cov)[1],
                                   rtol=1e-12, atol=1e-12)


# ---- 2. measured reference behaviour --------------------------------------------------------------------
@pytest.mark.needs_reference
def test_reference_edges():
    ref = reference()
    trainer = ref.ComplexCircularSymmetricGaussianTrainer()
    Model = ref.ComplexCircularSymmetricGaussian
    # D = 1 works
    y1 = oc.frames(3, (20, 1))
    m = trainer.fit(y1)
    assert m.covariance.shape == (1, 1) and np.isfinite(m.log_pdf(y1)).all()
    # result dtypes
    y64 = oc.frames(4, (2, 1, 30, 3), np.complex64)
    assert trainer.fit(y64).covariance.dtype == np.complex64
    s32 = oc.saliency(4, (2, 3, 30), np.float32)
    assert trainer.fit(y64, saliency=s32).covariance.dtype == np.complex64
    assert trainer.fit(y64, saliency=s32.astype(np.float64)).covariance.dtype == np.complex128
    # zero saliency: a zero covariance, which log_pdf refuses
    zero = trainer.fit(y64[0, 0], saliency=np.zeros(30, np.float32))
    assert (zero.covariance == 0).all()
    with pytest.raises(np.linalg.LinAlgError):
        zero.log_pdf(y64[0, 0])
    with pytest.raises(AssertionError):
        trainer.fit(y64.real)
    with pytest.raises(ValueError, match='Unknown covariance type'):
        trainer.fit(y64, covariance_type='diagonal')
    # the documented deviation: an indefinite Hermitian matrix gives numbers there
    lp = Model(covariance=np.diag([1.0, -2.0, 3.0]).astype(np.complex128)).log_pdf(
        oc.frames(5, (7, 3)))
    assert np.isfinite(lp).all()
    with pytest.raises(NotImplementedError):
        Model(covariance=np.stack([np.eye(3)] * 2)).sample((4,))


def test_host_side_behaviour_without_a_gpu():
    """What the device classes decide before any launch."""
    from pb_bss_amd.distribution import (ComplexCircularSymmetricGaussian,
                                         ComplexCircularSymmetricGaussianTrainer)
    trainer = ComplexCircularSymmetricGaussianTrainer()
    y = oc.frames(4, (2, 30, 3), np.complex64)
    with pytest.raises(AssertionError):
        trainer.fit(y.real)
    with pytest.raises(ValueError, match="Unknown covariance type 'diagonal'"):
        trainer.fit(y, covariance_type='diagonal')
    with pytest.raises(AssertionError):
        trainer.fit(y, saliency=np.ones((2, 29)))
    with pytest.raises(NotImplementedError, match='Not quite clear'):
        ComplexCircularSymmetricGaussian(covariance=np.stack([np.eye(3)] * 2)).sample((4,))
    np.random.seed(oc.SAMPLE_SEED)
    draws = ComplexCircularSymmetricGaussian(covariance=oc.sample_covariance()).sample(
        oc.SAMPLE_SIZE)
    assert draws.shape == (*oc.SAMPLE_SIZE, oc.SAMPLE_D)
    assert (draws == oc.fixtures()['sample']).all()


# ---- 3. the conditioning table -------------------------------------------------------------------------
def measured_log_pdf_error(cond):
    worst = 0.0
    for D in oc.CONDITION_DS:
        y, c = oc.conditioned(cond, D)
        xlp = oc.log_pdf_ext(y, c)[0]
        worst = max(worst, float(np.abs(oc.log_pdf(y, c) - xlp).max() / np.abs(xlp).max()))
    return worst


def test_log_pdf_error_of_the_oracle_per_conditioning_case():
    """The figures behind LOG_PDF_ORACLE_ERROR of the GPU file: what is written there must bound
    what is measured here (and by no more than a factor 4, so the table cannot be inflated)."""
    with open(os.path.join(HERE, 'test_gpu_ccsg.py')) as f:
        tree = ast.parse(f.read())
    table = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and n.targets[0].id == 'LOG_PDF_ORACLE_ERROR')
    assert sorted(table) == sorted(oc.CONDITIONS)
    for cond in oc.CONDITIONS:
        err = measured_log_pdf_error(cond)
        print(f'cond {cond:g}: oracle log-pdf error {err:.2e} max|log_pdf|')
        assert err <= table[cond] <= 4 * max(err, 1e-16), (cond, err, table[cond])
        assert f'{table[cond]:.1e}' in ast.get_docstring(tree)


def test_conditioning_cases_have_the_condition_they_claim():
    for cond in oc.CONDITIONS:
        for D in oc.CONDITION_DS:
            lam = np.linalg.eigvalsh(oc.conditioned(cond, D)[1])
            assert lam.min() > 0 and abs(lam.max() / lam.min() / cond - 1) < 1e-3, (cond, D)


# ---- 4. what the sweep reaches ----------------------------------------------------------------------------
def test_sweep_reaches_every_boundary_of_the_kernels():
    from pb_bss_amd import engine
    ds, ns, ks = set(oc.D_SWEEP), set(oc.N_SWEEP), set(oc.K_SWEEP)
    assert {1, 2, 3, 8, 9, 16, 33, 34} <= ds and min(ds) == 1 and max(ds) == engine.CCSG_MAX_D
    assert {1, 63, 64, 65, 257} <= ns and {1, 3, 7} <= ks and set(oc.B_SWEEP) == {1, 5}
    # both sides of every instantiation boundary of the log-pdf sweep
    assert engine.CCSG_SWEEP_D[-1] == engine.CCSG_MAX_D
    for bound in engine.CCSG_SWEEP_D[:-1]:
        assert bound in ds and bound + 1 in ds, bound
    # both sides of every frame-tile / span boundary, and of every change of the tile length
    lengths = {engine.ccsg_frames(D) for D in range(1, engine.CCSG_MAX_D + 1)}
    assert lengths == {engine.ccsg_frames(D) for D in ds}
    for D in range(1, engine.CCSG_MAX_D):
        if engine.ccsg_frames(D) != engine.ccsg_frames(D + 1):
            assert D in ds and D + 1 in ds, D
    for length in lengths:
        assert length in ns and length + 1 in ns, length
    for D in ds:  # ... met at every D: one tile exactly, and one frame over
        met = {N for N, *_ in oc.sweep_cases(D)}
        assert engine.ccsg_frames(D) in met and engine.ccsg_frames(D) + 1 in met, D
    # every class-tile length with K at it and one over; two tiles at D = 34
    for tile in {engine.ccsg_class_tile(D) for D in ds}:
        assert tile >= 1 and tile in ks and tile + 1 in ks, tile
    assert any(engine.ccsg_class_tile(34) < K <= 2 * engine.ccsg_class_tile(34) for K in ks)
    for D in ds:
        counts = {-(-K // engine.ccsg_class_tile(D)) for _, K, *_ in oc.sweep_cases(D)}
        assert {1, 2} <= counts, (D, counts)
        assert {K for _, K, *_ in oc.sweep_cases(D)} == ks
    # every dtype and saliency kind meets every D
    for D in ds:
        cases = oc.sweep_cases(D)
        assert {c[3] for c in cases} == set(oc.Y_DTYPES)
        assert {c[4] for c in cases} == set(oc.SALIENCIES)
        assert {c[2] for c in cases} == set(oc.B_SWEEP)


def test_class_tile_fits_the_lds():
    from pb_bss_amd import engine
    for D in range(1, engine.CCSG_MAX_D + 1):
        tile = engine.ccsg_class_tile(D)
        frames = engine.ccsg_frames(D) * (D | 1) * 16
        assert 1 <= tile <= engine.CCSG_MAX_CLASS_TILE
        assert frames + tile * (D * D * 16 + D * 8 + 16) <= engine.CCSG_LDS


# ---- 5. name closure ------------------------------------------------------------------------------------------
def test_every_name_of_the_reference_package_is_served():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tools'))
    try:
        from make_ccsg_golden import imported_names
    finally:
        sys.path.pop(0)
    with open(os.path.join(oc.GOLDEN, 'ccsg_names.txt')) as f:
        names = f.read().split()
    init = os.path.join(refshim.REFERENCE_ROOT, 'pb_bss', 'distribution', '__init__.py')
    if refshim.available():
        assert names == imported_names(init)
    assert 'ComplexCircularSymmetricGaussian' in names and len(names) >= 30
    import pb_bss_amd.distribution as dist
    missing = [n for n in names if not hasattr(dist, n)]
    assert not missing, missing
    assert {'ComplexCircularSymmetricGaussian', 'ComplexCircularSymmetricGaussianTrainer'} <= set(
        dist.__all__)
