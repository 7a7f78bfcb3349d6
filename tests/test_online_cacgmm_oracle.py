"""CPU: the NumPy restatement of the frame-recursive cACGMM mask estimator
(tests/oracle_online_cacgmm.py) against routes that do not share its arithmetic -- the same
recursion in numpy.clongdouble (its own error `e_case`), the batch covariance as a plain weighted
sum with numpy.linalg.inv / slogdet, the closed form of the counts, and oracle.cacgmm's predict of
the same model -- and the table of `e_case` committed in tests/test_gpu_online_cacgmm.py against a
fresh measurement.  Then the parts of the public interface that need no GPU."""
import functools

import numpy as np
import pytest

import oracle_online_cacgmm as oc
from test_gpu_online_cacgmm import E_CASE

EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def run(case, alpha):
    Y, state, B0 = oc.case_input(case)
    out = oc.recursive(Y, state, alpha, oc.EPS_AFF)
    return (Y, state, B0) + out


@pytest.mark.parametrize('case', oc.CASES, ids=str)
def test_committed_e_case_is_what_the_restatement_measures(case):
    """The largest over both input dtypes, per alpha; the committed table stays within a factor 4
    of it (a floor of 1e-16 for the entries that are all rounding of a few operations).  The
    conditions of the sweep: nothing flagged (measure_e_case asserts it), e_case <= 1e-12."""
    for alpha in oc.ALPHAS:
        runs = [oc.measure_e_case(case, alpha, dt) for dt in (np.complex128, np.complex64)]
        measured = np.max(np.array(runs), axis=0)
        print(case, alpha, ' '.join(f'{v:.1e}' for v in measured))
        assert measured.max() <= 1e-12, (case, alpha, measured)
        for have, want in zip(E_CASE[case, alpha], measured):
            assert max(want, 1e-16) / 4 <= max(have, 1e-16) <= 4 * max(want, 1e-16), (
                case, alpha, E_CASE[case, alpha], measured)


def test_table_covers_the_sweep():
    assert set(E_CASE) == {(c, a) for c in oc.CASES for a in oc.ALPHAS}
    assert set(oc.CASES) >= {(2, 2, 64), (3, 2, 65), (4, 3, 130), (5, 4, 33), (8, 3, 300),
                             (16, 8, 200), (2, 2, 1000), (2, 2, 31), (2, 2, 32), (2, 2, 33),
                             (9, 3, 70), (12, 5, 70), (4, 8, 40), (8, 8, 40)}
    assert oc.ALPHAS == (1.0, 0.999, 0.95) and oc.BATCH == 3
    # the frame tile the cases straddle is the kernel's, and the Python layer mirrors its plan
    import os
    import re
    from pb_bss_amd import engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'pb_bss_amd', 'csrc', 'online_cacgmm.hpp')) as f:
        plan = dict(re.findall(r'constexpr int (kOnlineCacgmm\w+) = (\d+);', f.read()))
    assert int(plan['kOnlineCacgmmTile']) == engine.ONLINE_CACGMM_TILE == oc.TILE
    assert int(plan['kOnlineCacgmmMaxD']) == engine.ONLINE_CACGMM_MAX_D == 16
    assert int(plan['kOnlineCacgmmMaxK']) == engine.ONLINE_CACGMM_MAX_K == 8
    # the recipe of the inputs
    case = (4, 3, 130)
    Y, (P0, L0, Lam0, pi0), B0 = oc.case_input(case)
    assert Y.shape == (3, 4, 130) and P0.shape == B0.shape == (3, 3, 4, 4)
    zero = (np.abs(Y) ** 2).sum(axis=1) == 0
    assert zero[:, oc.zero_frame(case)].all() and zero.sum() == oc.BATCH
    assert (pi0 == 1 / 3).all() and np.allclose(Lam0, 10 / 3)
    assert np.abs(P0 @ B0 - np.eye(4)).max() < 1e-12
    assert np.abs(L0 - np.linalg.slogdet(B0)[1]).max() == 0


@pytest.mark.parametrize('case', oc.CASES, ids=str)
def test_batch_route(case):
    """After T frames, with the recorded gamma and q, B_k is a plain exponentially weighted sum:
    P_k against its inverse within 16 cond eps (relative to max |P_k|, as P B = I within
    16 cond eps), L_k against its slogdet (an absolute error of D cond-free roundings per frame:
    (16 + T) D eps, relative to max(|L|, 1)), Lambda against its closed form ((16 + T) eps)."""
    D, K, T = case
    worst = 0.0
    for alpha in oc.ALPHAS:
        Y, state, B0, G, Q, P, L, Lam, pi, flagged = run(case, alpha)
        assert not flagged.any()
        for b in range(oc.BATCH):
            Bk, Lk = oc.batch_covariance(Y[b], G[b], Q[b], alpha, B0[b], state[2][b])
            cond = np.linalg.cond(Bk)
            assert cond.max() <= 1e5, (case, alpha, b, cond)
            assert np.abs(Lam[b] - Lk).max() <= (16 + T) * EPS * np.abs(Lk).max()
            for k in range(K):
                err = np.abs(P[b, k] @ Bk[k] - np.eye(D)).max()
                worst = max(worst, err / (16 * cond[k] * EPS))
                assert err <= 16 * cond[k] * EPS, (case, alpha, b, k, err, cond[k])
                inv = np.linalg.inv(Bk[k])
                assert np.abs(P[b, k] - inv).max() <= 16 * cond[k] * EPS * np.abs(inv).max()
            want = np.linalg.slogdet(Bk)[1]
            tol = (16 + T) * D * EPS * max(np.abs(want).max(), 1.0)
            assert np.abs(L[b] - want).max() <= tol, (case, alpha, b, np.abs(L[b] - want).max(), tol)
            assert np.abs(pi[b] - Lam[b] / Lam[b].sum()).max() <= 4 * EPS  # normalised counts
    print(f'{case}: worst {worst:.3f} of 16 cond eps')


def test_first_frame_is_the_offline_predict():
    """gamma and q of the first frame from a model's state are oracle.cacgmm's predict of that
    model on that frame, up to the clip (a handful of roundings: another product order)."""
    from oracle import cacgmm as ref
    for case in [(4, 3, 130), (8, 3, 300), (16, 8, 200), (2, 2, 64)]:
        D, K, T = case
        Y, state, B0 = oc.case_input(case)
        lam, vec = np.linalg.eigh(B0)
        model = dict(weight=state[3][..., None], eigvec=vec, eigval=lam)
        P0 = np.einsum('...de,...e,...ge->...dg', vec, 1 / lam, vec.conj())
        L0 = np.log(lam).sum(axis=-1)
        G, Q = oc.recursive(Y[:, :, :1], (P0, L0, state[2], state[3]), 0.95, 0.0)[:2]
        aff, q = ref.em_predict(model, Y[:, :, :1].swapaxes(1, 2), return_quadratic_form=True)
        cond = (lam.max(axis=-1) / lam.min(axis=-1)).max()
        assert np.abs(Q - q).max() <= 16 * cond * EPS * np.abs(q).max(), case
        assert np.abs(G - aff).max() <= 64 * D * cond * EPS, case
        assert np.abs(G.sum(axis=1) - 1).max() <= 8 * EPS


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_blocks_and_edges_of_the_restatement():
    case, alpha = (3, 2, 65), 0.95
    D, K, T = case
    Y, state, B0, G, Q, P, L, Lam, pi, flagged = run(case, alpha)
    assert not flagged.any()
    assert (P == P.conj().swapaxes(-1, -2)).all()
    assert (np.diagonal(P, axis1=-2, axis2=-1).imag == 0).all()
    assert (G >= oc.EPS_AFF).all() and (G <= 1 - oc.EPS_AFF).all()
    # blocks of any lengths, each continuing from the state of the one before: bit for bit
    st, gs, qs, t0 = state, [], [], 0
    for n in (1, 1, 7, 33, 65 - 42):
        out = oc.recursive(Y[:, :, t0:t0 + n], st, alpha, oc.EPS_AFF)
        st = out[2:6]
        gs.append(out[0])
        qs.append(out[1])
        t0 += n
    assert same(np.concatenate(gs, axis=-1), G) and same(np.concatenate(qs, axis=-1), Q)
    assert all(same(a, b) for a, b in zip(st, (P, L, Lam, pi)))
    # the zero frame returns pi and leaves the state untouched
    z = oc.zero_frame(case)
    before = oc.recursive(Y[:, :, :z], state, alpha, oc.EPS_AFF)
    upto = oc.recursive(Y[:, :, :z + 1], state, alpha, oc.EPS_AFF)
    assert same(upto[0][:, :, z], before[5]) and (upto[1][:, :, z] == 0).all()
    assert all(same(a, b) for a, b in zip(upto[2:6], before[2:6]))
    assert same(G[:, :, z], before[5])
    # update_weight = False: pi never changes
    fixed = oc.recursive(Y, state, alpha, oc.EPS_AFF, update_weight=False)
    assert same(fixed[5], state[3]) and not fixed[6].any() and not same(fixed[0], G)
    assert not same(pi, state[3])
    # an indefinite initial precision: flagged at the first frame, NaN from there on
    Pbad = state[0].copy()
    Pbad[1, 0] = -Pbad[1, 0]
    bad = oc.recursive(Y, (Pbad,) + state[1:], alpha, oc.EPS_AFF)
    assert bad[6].tolist() == [False, True, False]
    assert np.isnan(bad[0][1]).all() and np.isnan(bad[1][1]).all()
    assert all(np.isnan(a[1]).all() for a in bad[2:6])
    assert same(bad[0][[0, 2]], G[[0, 2]]) and same(bad[2][[0, 2]], P[[0, 2]])
    # a NaN sample in frame 30: the frames before are the clean run's
    N = Y.copy()
    N[0, 1, 30] = np.nan
    nn = oc.recursive(N[0], tuple(a[0] for a in state), alpha, oc.EPS_AFF)
    assert nn[6] and same(nn[0][:, :30], G[0, :, :30]) and np.isnan(nn[0][:, 30:]).all()
    assert np.isnan(nn[1][:, 30:]).all() and all(np.isnan(a).all() for a in nn[2:6])


def test_public_names_and_refusals_without_a_gpu():
    from pb_bss_amd import distribution, engine
    from pb_bss_amd.distribution import CACGMM, ComplexAngularCentralGaussian
    from pb_bss_amd.distribution import online_cacgmm as mod
    for name in ('recursive_cacgmm', 'OnlineCACGMM', 'OnlineCACGMMState'):
        assert name in distribution.__all__ and getattr(distribution, name) is getattr(mod, name)
    assert engine.ONLINE_CACGMM_MAX_D == 16 and engine.ONLINE_CACGMM_MAX_K == 8

    def model(D, K, weight_shape=None, lead=(5,)):
        vec = np.broadcast_to(np.eye(D, dtype=np.complex128), lead + (K, D, D)).copy()
        val = np.ones(lead + (K, D))
        weight = np.full(lead + (K, 1) if weight_shape is None else weight_shape, 1.0 / K)
        return CACGMM(weight=weight, cacg=ComplexAngularCentralGaussian(vec, val))
    Y = np.zeros((5, 4, 10), np.complex64)
    with pytest.raises(ValueError, match='exactly one'):
        distribution.recursive_cacgmm(Y)
    with pytest.raises(ValueError, match='exactly one'):
        distribution.recursive_cacgmm(Y, model(4, 2), state=object())
    with pytest.raises(ValueError, match='layout'):
        distribution.recursive_cacgmm(Y, model(4, 2), layout='t f d')
    for shape in [(5, 2), (2,), (5, 1, 2, 10), (5, 2, 10), (5, 3, 1)]:
        with pytest.raises(ValueError, match=r'\(\.\.\., K, 1\)'):
            distribution.OnlineCACGMMState.from_model(model(4, 2, shape))
    with pytest.raises(ValueError, match='initial_count'):
        distribution.OnlineCACGMMState.from_model(model(4, 2), initial_count=0.0)
    with pytest.raises(NotImplementedError, match='ONLINE_CACGMM_MAX_D = 16'):
        distribution.OnlineCACGMMState.from_model(model(17, 2))
    with pytest.raises(NotImplementedError, match='ONLINE_CACGMM_MAX_K = 8'):
        distribution.OnlineCACGMMState.from_model(model(4, 9))
    with pytest.raises(NotImplementedError, match='ONLINE_CACGMM_MAX_K = 8'):
        distribution.OnlineCACGMM(model(4, 9))
    with pytest.raises(ValueError):
        distribution.OnlineCACGMMState.from_model(model(4, 1))
    for alpha in (0.0, -0.5, 1.5, float('nan')):
        with pytest.raises(AssertionError):
            distribution.recursive_cacgmm(Y, model(4, 2), alpha=alpha)
    with pytest.raises(AssertionError):
        distribution.recursive_cacgmm(Y, model(4, 2), affiliation_eps=-1e-3)
