"""CPU: the NumPy restatement of the frame-recursive MVDR beamformer
(tests/oracle_online_beamformer.py) against routes that do not share its arithmetic -- the same
recursion in numpy.clongdouble (its own error `e_case`) and the batch solution from plain weighted
sums and numpy.linalg.solve -- and the table of `e_case` committed in
tests/test_gpu_online_beamformer.py against a fresh measurement."""
import numpy as np
import pytest

import oracle_online_beamformer as oo
from test_gpu_online_beamformer import E_CASE

EPS = 2.0 ** -52


@pytest.mark.parametrize('case', oo.CASES, ids=str)
def test_committed_e_case_is_what_the_restatement_measures(case):
    """The largest over both input dtypes, per alpha; the committed table stays within a factor 4
    of it (a floor of 1e-16 for the entries that are all rounding of a few operations)."""
    for alpha in oo.ALPHAS:
        runs = [oo.measure_e_case(case, alpha, dt) for dt in (np.complex128, np.complex64)]
        measured = np.max(np.array(runs), axis=0)
        print(case, alpha, ' '.join(f'{v:.1e}' for v in measured))
        for have, want in zip(E_CASE[case, alpha], measured):
            assert max(want, 1e-16) / 4 <= max(have, 1e-16) <= 4 * max(want, 1e-16), (
                case, alpha, E_CASE[case, alpha], measured)


def test_table_covers_the_sweep():
    assert set(E_CASE) == {(c, a) for c in oo.CASES for a in oo.ALPHAS}
    assert set(oo.CASES) >= {(1, 8), (2, 64), (3, 65), (4, 130), (5, 33), (8, 300), (16, 200),
                             (2, 1000), (2, oo.TILE - 1), (2, oo.TILE), (2, oo.TILE + 1),
                             (2, 2 * oo.TILE)}
    assert {9, 12} <= {c[0] for c in oo.CASES}
    assert oo.ALPHAS == (1.0, 0.999, 0.95) and oo.BATCH == 3 and oo.P0 == 0.1
    assert all(oo.ref_channel(c) == c[0] - 1 for c in oo.CASES)
    # the frame tile the cases straddle is the kernel's, and the Python layer mirrors its plan
    import os
    import re
    from pb_bss_amd import engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'pb_bss_amd', 'csrc', 'online_bf.hpp')) as f:
        plan = dict(re.findall(r'constexpr int (kOnlineBf\w+) = (\d+);', f.read()))
    assert int(plan['kOnlineBfTile']) == engine.ONLINE_BF_TILE == oo.TILE
    assert int(plan['kOnlineBfMaxD']) == engine.ONLINE_BF_MAX_D == 16
    Y, s, v = oo.case_input((4, 130))
    assert (s[:, 0::7] == 0).all() and (v[:, 3::11] == 0).all()
    assert (s >= 0).all() and (s <= 1).all() and (v >= 0).all()
    keep = np.ones(130, bool)
    keep[3::11] = False
    assert (v[:, keep] == 1.0 - s[:, keep]).all()


@pytest.mark.parametrize('case', oo.CASES, ids=str)
def test_batch_equivalence(case):
    """After T frames Phi and Psi^-1 are the exponentially weighted sums and the last vector is
    their Souden solution.  The recursion rounds the statistics once or twice per frame, at worst
    T eps relative in all (the sums themselves: 16 eps of slack for their own D-term and T-term
    rounding); a relative perturbation delta of the statistics moves Psi^-1 and the solution by
    cond delta.  Hence (16 + T) eps for Phi and cond (16 + T) eps for Psi^-1 and w."""
    D, T = case
    r = oo.ref_channel(case)
    worst = 0.0
    for alpha in oo.ALPHAS:
        Y, s, v = oo.case_input(case)
        X, W, Phi, Psi, flagged = oo.recursive(Y, s, v, alpha, r, oo.P0)
        assert not flagged.any() and np.isfinite(X).all() and np.isfinite(W).all()
        assert (W[0] == 0).all() and (X[:, 0] == 0).all()     # Phi is still 0 at the first frame
        for b in range(oo.BATCH):
            P, N = oo.batch_statistics(Y[b], s[b], v[b], alpha, oo.P0)
            w, cond = oo.batch_souden(P, N, r)
            assert cond <= 1e4, cond
            tol = (16 + T) * EPS
            assert np.abs(Phi[b] - P).max() <= tol * np.abs(P).max()
            assert np.abs(np.linalg.inv(Psi[b]) - N).max() <= cond * tol * np.abs(N).max()
            err = np.abs(W[-1, b] - w).max() / np.abs(w).max()
            worst = max(worst, err / (cond * EPS))
            assert err <= cond * tol, (case, alpha, b, err, cond)
    print(f'{case}: worst {worst:.3f} of cond eps')


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_blocks_and_edges_of_the_restatement():
    case, alpha = (3, 65), 0.95
    r = oo.ref_channel(case)
    Y, s, v = oo.case_input(case)
    X, W, Phi, Psi, flagged = oo.recursive(Y, s, v, alpha, r, oo.P0)
    assert not flagged.any()
    for M in (Phi, Psi):
        assert (M == M.conj().swapaxes(-1, -2)).all()
        assert (np.diagonal(M, axis1=-2, axis2=-1).imag == 0).all()
    # blocks of any lengths, each continuing from the state of the one before: bit for bit
    state, xs, ws, t0 = None, [], [], 0
    for n in (1, 1, 7, 33, 65 - 42):
        x, w, P, Q, _ = oo.recursive(Y[:, :, t0:t0 + n], s[:, t0:t0 + n], v[:, t0:t0 + n], alpha,
                                     r, oo.P0, state=state)
        state = (P, Q)
        xs.append(x)
        ws.append(w)
        t0 += n
    assert same(np.concatenate(xs, axis=-1), X) and same(np.concatenate(ws, axis=0), W)
    assert same(state[0], Phi) and same(state[1], Psi)
    # all-zero masks: x = 0 and nothing flagged at alpha = 1, Psi stays I / p0
    Z = oo.recursive(Y, 0 * s, 0 * v, 1.0, r, oo.P0)
    assert not Z[4].any() and (Z[0] == 0).all() and (Z[1] == 0).all() and (Z[2] == 0).all()
    assert (Z[3] == np.eye(3) / oo.P0).all()
    # an inf sample: flagged, NaN from that frame on, the frames before are the clean run's
    N = Y[0].copy()
    N[1, 30] = np.inf
    Xn, Wn, Pn, Qn, flag = oo.recursive(N, s[0], v[0], alpha, r, oo.P0)
    assert flag and np.isnan(Xn[30:]).all() and np.isnan(Wn[30:]).all()
    assert same(Xn[:30], X[0, :30]) and same(Wn[:30], W[:30, 0])
    assert np.isnan(Pn).all() and np.isnan(Qn).all()
    # the known limit: alpha < 1 and no noise-mask mass, Psi grows like alpha^-t into the flag
    T = 1200
    G = oo.recursive(np.ones((2, T)), np.ones(T), np.zeros(T), 0.5, 0, 1.0)
    assert G[4] and np.isfinite(G[0][:1000]).all() and np.isnan(G[0][-1])
