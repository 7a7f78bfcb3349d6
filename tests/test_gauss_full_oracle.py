"""CPU: the premises of tests/test_gpu_gauss_full.py.

1. On every hard input of tests/oracle_gauss_full.py the float64 oracle
   (`oracle.embed.gaussian_fit(..., 'full')`) agrees with its longdouble restatement: covariance
   within 1e-13 max|cov|, mean within 1e-13 of its own scale max(max|mean|, sqrt(max|cov|)) (the
   covariance bound carries the square of the data's unit; the mean of rows at 1e6 is not even
   representable to 1e-13 max|cov|).  Only then may the oracle serve as the GPU tests' reference.
2. The oracle's log-pdf error against the longdouble one, relative to max|log_pdf|, per
   conditioning case: printed under `pytest -s`, copied into the GPU file's docstring, and the
   GPU file's table is checked to bound what is measured here.
3. The E list of the GPU shape test reaches every variant of the workgroup Cholesky on both
   sides of each boundary and every tile count with E + 1 exact and one over.
"""
import numpy as np
import pytest

import oracle_gauss_full as og
from oracle import embed as oe


@pytest.mark.parametrize('name', sorted(og.hard_cases()))
def test_float64_oracle_matches_extended_precision_on_hard_input(name):
    y, w = og.hard_cases()[name]
    mean, cov = oe.gaussian_fit(y[None], w, 'full')
    xmean, xcov = og.fit_ext(y, w)
    scale = float(np.abs(xcov).max())
    mscale = max(float(np.abs(xmean).max()), np.sqrt(scale))
    cerr = float(np.abs(cov - xcov).max())
    merr = float(np.abs(mean - xmean).max())
    print(f'{name}: cov err {cerr / scale if scale else cerr:.1e} max|cov|, '
          f'mean err {merr / mscale if mscale else merr:.1e} of its scale')
    assert cerr <= 1e-13 * scale
    assert merr <= 1e-13 * mscale
    if name == 'empty_class':
        assert (mean[1] == 0).all() and (cov[1] == 0).all()


def test_nan_in_a_weightless_row_reaches_the_oracle_covariance():
    y, w = og.nan_row(0)
    mean, cov = oe.gaussian_fit(y[None], w, 'full')
    assert np.isnan(mean[:, 3]).all() and np.isnan(cov[:, 3, :]).all()
    assert np.isfinite(np.delete(np.delete(cov, 3, 1), 3, 2)).all()


def measured_log_pdf_error(cond):
    y, w = og.conditioned(cond)
    mean, cov = oe.gaussian_fit(y[None], w, 'full')
    lp = oe.gaussian_log_pdf(y[None], mean, cov, 'full')
    xlp = og.log_pdf_ext(y, mean, cov)
    return float(np.abs(lp - xlp).max() / np.abs(xlp).max())


def test_log_pdf_error_of_the_oracle_per_conditioning_case():
    """The figures behind LOG_PDF_ORACLE_ERROR of the GPU file: what is written there must bound
    what is measured here (and by no more than a factor 4, so the table cannot be inflated)."""
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                            'test_gpu_gauss_full.py')).read()
    tree = ast.parse(src)
    table = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and n.targets[0].id == 'LOG_PDF_ORACLE_ERROR')
    for cond in (1e2, 1e6, 1e10):
        err = measured_log_pdf_error(cond)
        print(f'cond {cond:g}: oracle log-pdf error {err:.2e} max|log_pdf|')
        assert err <= table[cond] <= 4 * max(err, 1e-16), (cond, err, table[cond])
        assert f'{table[cond]:.1e}' in ast.get_docstring(tree)


def test_log_pdf_is_the_reference_form_not_the_textbook_one():
    y, w = og.conditioned(1e2)
    mean, cov = oe.gaussian_fit(y[None], w, 'full')
    lp = oe.gaussian_log_pdf(y[None], mean, cov, 'full')
    d = y - mean[0]
    textbook = (-0.5 * y.shape[1] * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(cov[0])[1]
                - 0.5 * np.einsum('nd,dD,nD->n', d, np.linalg.inv(cov[0]), d))
    assert np.abs(lp[0] - textbook).max() > 1e-3 * np.abs(lp[0]).max()


def test_shape_sweep_reaches_every_cholesky_variant_and_tile_count():
    es = set(og.E_SWEEP)
    assert max(es) == 63 and min(es) == 1 and {1, 2, 3, 4} <= es
    assert {og.chol_positions(E) for E in es} == set(range(1, 9))
    for q in range(1, 8):  # both sides of the boundary between Q = q and q + 1
        last = max(E for E in range(1, 64) if og.chol_positions(E) == q)
        assert last in es and last + 1 in es, (q, last)
        assert og.chol_positions(last + 1) == q + 1
    for t in range(1, 5):
        assert 16 * t - 1 in es, t            # E + 1 = 16 t exactly
        assert og.tiles(16 * t - 1) == t
        if t < 4:
            assert 16 * t in es, t            # one over: the next tile holds the 1 alone
            assert og.tiles(16 * t) == t + 1
