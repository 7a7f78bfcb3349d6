"""CPU: the NumPy restatement of frame-recursive WPE (tests/oracle_wpe_online.py) against routes
that do not share its arithmetic -- the same recursion in numpy.clongdouble (its own error
`e_case`) and the batch solution of the exponentially weighted normal equations -- and the table
of `e_case` committed in tests/test_gpu_wpe_online.py against a fresh measurement."""
import numpy as np
import pytest

import oracle_wpe_online as oo
from test_gpu_wpe_online import E_CASE

EPS = 2.0 ** -52


@pytest.mark.parametrize('case', oo.CASES, ids=str)
def test_committed_e_case_is_what_the_restatement_measures(case):
    """The largest over both input dtypes and the causal / given power, per alpha; the committed
    table stays within a factor 4 of it (a floor of 1e-16 for the entries that are all rounding
    of a few operations)."""
    for alpha in oo.ALPHAS:
        runs = [oo.measure_e_case(case, alpha, dt, given)
                for dt in (np.complex128, np.complex64) for given in (False, True)]
        measured = np.max(np.array(runs), axis=0)
        print(case, alpha, ' '.join(f'{v:.1e}' for v in measured))
        for have, want in zip(E_CASE[case, alpha], measured):
            assert max(want, 1e-16) / 4 <= max(have, 1e-16) <= 4 * max(want, 1e-16), (
                case, alpha, E_CASE[case, alpha], measured)


def test_table_covers_the_sweep():
    assert set(E_CASE) == {(c, a) for c in oo.CASES for a in oo.ALPHAS}
    assert set(oo.CASES) >= {(1, 1, 1, 8), (2, 3, 1, 64), (3, 3, 2, 65), (4, 5, 3, 130),
                             (6, 10, 3, 300), (8, 10, 3, 300), (16, 6, 3, 200), (8, 12, 3, 257),
                             (2, 3, 1, 1000)}
    assert oo.ALPHAS == (1.0, 0.9999, 0.99) and oo.BATCH == 3


@pytest.mark.parametrize('case', [c for c in oo.CASES if c[3] > 8], ids=str)
def test_filter_is_the_batch_solution(case):
    """G after T frames is (alpha^T I + R)^-1 C of the offline restatement's correlations with
    the weights alpha^(T - 1 - t) / lambda_t: both routes are backward stable, so they agree to
    about cond eps."""
    D, taps, delay, T = case
    worst = 0.0
    for alpha in oo.ALPHAS:
        for given in (False, True):
            Y = oo.case_input(case)
            pw = oo.case_power(case) if given else None
            G = oo.recursive(Y, taps, delay, alpha, pw)[2]
            for b in range(oo.BATCH):
                lam = pw[b] if given else oo.causal_power(Y[b], taps, delay)
                Gw, cond = oo.batch_filter(Y[b], lam, taps, delay, alpha)
                err = np.abs(G[b] - Gw).max() / np.abs(Gw).max()
                worst = max(worst, err / (cond * EPS))
                assert err <= 16 * cond * EPS, (case, alpha, given, b, err, cond)
    print(f'{case}: worst {worst:.3f} of cond eps')


def test_the_mirror_is_what_keeps_the_recursion_from_drifting():
    """(2, 3, 1, 1000), alpha = 0.99: the antisymmetric rounding residue of the full-matrix
    update is divided by alpha every frame; with the mirror the float64 run stays at rounding
    level of its longdouble run."""
    case, alpha = (2, 3, 1, 1000), 0.99
    D, taps, delay, T = case
    Y = oo.case_input(case)
    exact = oo.recursive(Y, taps, delay, alpha, ctype=np.clongdouble)[0]
    scale = np.abs(exact).max()
    mirrored = np.abs(oo.recursive(Y, taps, delay, alpha)[0] - exact).max() / scale
    textbook = np.abs(oo.recursive(Y, taps, delay, alpha, mirror=False)[0] - exact).max() / scale
    print(f'mirrored {mirrored:.1e}, textbook {textbook:.1e}')
    assert mirrored <= 64 * EPS
    assert textbook >= 100 * mirrored
    # the mirror changes nothing in exact arithmetic: the longdouble runs agree
    loose = oo.recursive(Y, taps, delay, alpha, ctype=np.clongdouble, mirror=False)[0]
    assert np.abs(loose - exact).max() / scale <= 1e-13


def test_blocks_and_edges_of_the_restatement():
    Y = oo.case_input((2, 3, 1, 64))
    X, P, G, flagged = oo.recursive(Y, 3, 1, 0.99)
    assert not flagged.any() and np.isfinite(X).all()
    assert (P == P.conj().swapaxes(-1, -2)).all()
    assert (np.diagonal(P, axis1=-2, axis2=-1).imag == 0).all()
    # the first frame has no past: x_0 = y_0; the causal power of frame 0 is its own
    assert (X[:, :, 0] == Y[:, :, 0]).all()
    lam = oo.causal_power(Y[0], 3, 1)
    assert np.isclose(lam[0], np.mean(np.abs(Y[0, :, 0]) ** 2))
    assert np.isclose(lam[10], np.mean(np.abs(Y[0, :, 6:11]) ** 2))
    # zeros: gain 0, P only divided by alpha
    Z = oo.recursive(np.zeros((2, 5), np.complex128), 3, 1, 0.5)
    assert (Z[0] == 0).all() and (Z[2] == 0).all() and (Z[1] == 32 * np.eye(6)).all()
    # a NaN frame: flagged, NaN from that frame on
    N = Y[0].copy()
    N[0, 30] = np.nan
    Xn, Pn, Gn, flag = oo.recursive(N, 3, 1, 0.99)
    assert flag and np.isnan(Xn[:, 30:]).all() and (Xn[:, :30] == X[0, :, :30]).all()
    assert np.isnan(Pn).all() and np.isnan(Gn).all()
