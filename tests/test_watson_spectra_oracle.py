"""CPU: the inputs of tests/test_gpu_cwmm_spectra.py do what they promise.

tests/oracle_watson_spectra.py builds frames with a prescribed covariance spectrum; the GPU tests
rely on what the ORACLE does with them over the first EM iterations -- the gap between the two
leading eigenvalues of class 0, the distance of that pair to the rest, a mode that jumps.  Those
properties are asserted here from `trajectory`, for every sensor count the GPU tests use, and the
figures are printed (pytest -s).
"""
import numpy as np
import pytest

import oracle_watson_spectra as ws
from oracle import cwmm as ow

TS = (192, 320)


@pytest.mark.parametrize('D', ws.ALL_D)
def test_block_has_the_prescribed_covariance(D):
    """block(): unit-norm frames, mean outer product U diag(lam) U^H (measured at D = 6, T = 96:
    covariance 1.1e-16, norm 2.2e-16).  Bound: (D + 8) eps -- every frame component is a D-term
    product sum, the outer products and their mean add a few roundings of entries <= 1."""
    bound = (D + 8) * np.finfo(np.float64).eps
    rng = np.random.default_rng(D)
    for T in (D, 96, 160):
        lam = rng.uniform(0.1, 1.0, D)
        lam[-1] = 0.0  # a singular covariance is as exact as any other
        lam /= lam.sum()
        U = ws.unitary(D, D + T)
        assert np.abs(U.conj().T @ U - np.eye(D)).max() < bound
        y = ws.block(U, lam, T)
        cov = np.einsum('td,te->de', y, y.conj()) / T
        err_c = np.abs(cov - (U * lam) @ U.conj().T).max()
        err_n = np.abs(np.linalg.norm(y, axis=-1) - 1).max()
        print(f'block D={D} T={T}: covariance {err_c:.1e}, norm {err_n:.1e}')
        assert err_c < bound and err_n < bound
    with pytest.raises(AssertionError):
        ws.block(ws.unitary(D, 0), np.full(D, 1.0 / D), D - 1)


def test_trajectory_is_the_loop_of_cwmm_fit():
    """trajectory() restates nothing: its last model is cwmm_fit's bit for bit, and
    covariance_after(model of iteration i) is the covariance iteration i + 1 worked on."""
    Y, init, p = ws.mode_jump(0.3, D=5, T=192)
    tr = p['trajectory']
    ref = ow.cwmm_fit(Y, init, iterations=len(tr))
    for key in ('weight', 'mode', 'concentration'):
        assert np.array_equal(tr[-1][key], ref[key]), key
    for i in range(len(tr) - 1):
        assert np.abs(ws.covariance_after(tr[i], Y) - tr[i + 1]['covariance']).max() < 1e-15
    shared = ws.trajectory(Y, init, 3, weight_constant_axis=(-3, -1))
    ref = ow.cwmm_fit(Y, init, iterations=3, weight_constant_axis=(-3, -1))
    assert shared[-1]['weight'].shape == (1, 2, 1)
    assert np.array_equal(shared[-1]['concentration'], ref['concentration'])


@pytest.mark.parametrize('D', ws.NEAR_DEGENERATE_D)
def test_first_covariance_is_a_convex_combination_of_the_blocks(D):
    """With an affiliation that is constant within a block the spectrum is set directly: class 0
    of near_degenerate(g) starts from 0.9 (0.4, 0.4 - g, flat) + 0.1 (flat, ..., 0.1, 0.7)."""
    for g in ws.GAPS:
        _, _, p = ws.near_degenerate(g, D=D, iterations=1)
        want = 0.9 * ws.flat_spectrum([0.4, 0.4 - g], D) + 0.1 * ws.flat_spectrum([0.7, 0.1], D)[::-1]
        got = p['trajectory'][0]['eigenvalues'][:, 0]
        assert np.abs(got - np.sort(want)).max() < 1e-15, (g, got, want)
        assert abs(p['per_iteration'][0]['gap_min'] - 0.9 * g) < 1e-15


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('D', ws.NEAR_DEGENERATE_D)
def test_near_degenerate_promises(D, T):
    """Every g: the first top gap of class 0 is 0.9 g to rounding; over the first three iterations
    the leading pair stays >= 0.05 above the third eigenvalue and the concentration is an
    ordinary one.  g >= 1e-5: the gap stays within [0.85 g, 1.05 g] over those iterations and
    consecutive modes agree to 1e-7 in overlap.  g = 1e-6: the gap holds at iterations 0 and 1
    (what the device A/B works on); from iteration 2 on the oracle's own mode is decided by its
    rounding at D <= 6 (1 - overlap 2e-3, 1e-5, 3e-7 at D = 4, 5, 6).  g = 1e-9: still within
    1e-8 at iteration 1.  g = 0: degenerate at iteration 0 only -- whichever vector of the plane
    the eigensolver returns, the E-step favours the frames along it and the covariance of
    iteration 1 has that vector on top with a gap of 3e-4 .. 2e-2 (printed)."""
    for g in ws.GAPS:
        _, _, p = ws.near_degenerate(g, D=D, T=T)
        per = p['per_iteration']
        print(f'near_degenerate g={g:g} D={D} T={T}: gap/g ' +
              ' '.join(f"{q['gap_min'] / max(g, 1e-300):.3f}..{q['gap_max'] / max(g, 1e-300):.3f}"
                       for q in per[:3]) if g >= 1e-6 else
              f'near_degenerate g={g:g} D={D} T={T}: gap ' +
              ' '.join(f"{q['gap_min']:.1e}..{q['gap_max']:.1e}" for q in per[:2]),
              '| sep ' + ' '.join(f"{q['sep_min']:.3f}" for q in per[:3]),
              '| 1-overlap ' + ' '.join(f"{1 - q['overlap_min']:.1e}" for q in per[1:3]),
              f"| kappa {min(q['conc_min'] for q in per):.1f}..{max(q['conc_max'] for q in per):.1f}")
        assert abs(per[0]['gap_max'] - 0.9 * g) < 1e-15, per[0]
        for q in per[:3]:
            assert q['sep_min'] >= 0.05, (g, q)
            assert 1.0 < q['conc_min'] <= q['conc_max'] < 30.0, (g, q)
        for q in per[:3] if g >= 1e-5 else per[:2] if g >= 1e-6 else []:
            assert 0.85 * g <= q['gap_min'] <= q['gap_max'] <= 1.05 * g, (g, q)
        if g >= 1e-5:
            for q in per[:3]:
                assert 1 - q['overlap_min'] < 1e-7, (g, q)
        if g == 1e-9:
            assert per[1]['gap_max'] <= 1e-8, per[1]


ISSUE_GAPS_D6 = {0.2: 0.052, 0.3: 0.044, 0.4: 0.030, 0.5: 0.0073}


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('D', ws.MODE_JUMP_D)
def test_mode_jump_promises(D, T):
    """At iteration `jump_at` (1 or 2) the oracle's class-0 mode is orthogonal to the previous one
    in every bin (overlap < 0.5 asserted, 1e-14 measured), the new leading eigenvalue is alone
    (gap >= 1e-3 asserted, 2.8e-3 the smallest; the device mode is compared with that eigenvector
    at 1 - 1e-10 in overlap, which a 1e-9 error of the covariance allows from a gap of 7e-5 on:
    (1e-9 / gap)^2 / 2) and the second eigenvalue --
    the one the stale vector belongs to -- is >= 0.05 above the third."""
    for share in ws.SHARES:
        _, _, p = ws.mode_jump(share, D=D, T=T)
        n, per = p['jump_at'], p['per_iteration']
        print(f'mode_jump share={share} D={D} T={T}: jump at {n}, overlap there '
              f"{per[n]['overlap_max']:.1e}, gap {per[n]['gap_min']:.4f}, second-to-third "
              f"{per[n]['sep_min']:.3f}, gaps " + ' '.join(f"{q['gap_min']:.4f}" for q in per))
        assert n in (1, 2), n
        assert per[n]['overlap_max'] < 0.5
        assert per[n]['gap_min'] >= 1e-3 and per[n]['sep_min'] >= 0.05, per[n]
        for q in per[:n]:  # no earlier jump, the start is a settled mode
            assert q['overlap_min'] > 1 - 1e-10, q
        if D == 6:
            assert n == 1 and abs(per[1]['gap_min'] / ISSUE_GAPS_D6[share] - 1) < 0.05, per[1]
            assert abs(per[3]['gap_min'] - 0.06) < 0.005, per[3]


@pytest.mark.parametrize('D', ws.ALL_D)
def test_one_class_scenarios(D):
    """isotropic / rank_one (K = 1): the covariance is the block's at every iteration; all
    eigenvalues 1 / D and concentration 0 (below the spline's range), or one eigenvalue 1 (to
    (D - 1) 1e-12) and the concentration at its cap."""
    for T in TS:
        _, init, p = ws.isotropic(D=D, T=T)
        assert init.shape[1] == 1
        for s in p['trajectory']:
            assert np.abs(s['eigenvalues'] - 1.0 / D).max() < (D + 8) * np.finfo(np.float64).eps
            assert (s['concentration'] == 0).all() and (s['affiliation'] == 1).all()
        _, _, p = ws.rank_one(D=D, T=T)
        for s in p['trajectory']:
            ev = s['eigenvalues'][:, 0]
            assert np.abs(ev[:, -1] - 1).max() < 1e-11 and np.abs(ev[:, :-1]).max() < 1.1e-12
            assert np.abs(ev[1::2, :-1]).max() < 64 * np.finfo(np.float64).eps  # exact variant
            assert (s['concentration'] == 500).all()
        assert p['per_iteration'][1]['overlap_min'] > 1 - 1e-12


@pytest.mark.parametrize('D', ws.ALL_D)
def test_empty_class_scenario(D):
    """The emptied class's first covariance is 0 / 0 (the device reports the status bit), the
    other bins are an ordinary two-class problem."""
    for T in TS:
        Y, init, p = ws.empty_class(D=D, T=T)
        e = p['empty_bin']
        assert (init[e, 1] == 0).all() and (init[e, 0] == 1).all() and len(p['keep']) == 3
        assert (init[p['keep']] > 0).all()
        for s in p['trajectory']:
            assert np.isfinite(s['mode']).all() and (s['concentration'] > 0).all()
        with np.errstate(all='ignore'):
            cov = ws.class_covariance(Y, init)
        assert np.isnan(cov[e, 1]).all() and np.isfinite(cov[e, 0]).all()
        assert np.isfinite(cov[p['keep']]).all()


@pytest.mark.parametrize('T', TS)
def test_whole_trajectory_comparisons_are_well_posed(T):
    """The oracle's own error (self_spread: same model, other roundings) after 4 iterations is
    below 1e-9 in the affiliations for every case the GPU file compares at 1e-7, and the reason
    near_degenerate(1e-5) is compared at D = 7, 8 only: measured at D = 4, 5, 6 it is 8e-4 .. 2e-3,
    8e-6 .. 3e-5 and 6e-8 .. 1e-7 -- EM itself amplifies a rotation inside the near-degenerate plane,
    the reference is NOT accurate to eps / g there."""
    for g, D in ws.PARITY_NEAR_DEGENERATE:
        Y, init, _ = ws.near_degenerate(g, D=D, T=T, iterations=1)
        aff, conc = ws.self_spread(Y, init, 4)
        print(f'self_spread near_degenerate g={g:g} D={D} T={T}: aff {aff:.1e} conc {conc:.1e}')
        assert aff < 1e-9 and conc < 1e-10, (g, D, aff, conc)
    for share, D in ws.PARITY_MODE_JUMP:
        Y, init, _ = ws.mode_jump(share, D=D, T=T, iterations=1)
        aff, conc = ws.self_spread(Y, init, 4)
        print(f'self_spread mode_jump share={share} D={D} T={T}: aff {aff:.1e} conc {conc:.1e}')
        assert aff < 1e-9 and conc < 1e-10, (share, D, aff, conc)
    for D in (4, 5, 6):
        Y, init, _ = ws.near_degenerate(1e-5, D=D, T=T, iterations=1)
        print(f'self_spread near_degenerate g=1e-05 D={D} T={T} (not compared): aff %.1e conc %.1e'
              % ws.self_spread(Y, init, 4))
    for kind in ('near_degenerate', 'mode_jump'):
        Y, init, _ = getattr(ws, kind)(1e-3 if kind == 'near_degenerate' else 0.3, D=6, F=5, T=T,
                                       iterations=1)
        aff, conc = ws.self_spread(Y, init, 4, weight_constant_axis=(-3, -1))
        print(f'self_spread {kind} shared weights T={T}: aff {aff:.1e} conc {conc:.1e}')
        assert aff < 1e-9 and conc < 1e-10


def test_dropped_sensor_counts_are_few_and_explained():
    pairs = [(s, D) for s in ws.SCENARIOS for D in ws.ALL_D]
    assert set(ws.DROPPED) <= set(pairs)
    assert len(ws.DROPPED) <= len(pairs) / 10, (len(ws.DROPPED), len(pairs))
    for pair, reason in ws.DROPPED.items():
        assert len(reason) > 40, pair
        with pytest.raises(AssertionError):
            getattr(ws, pair[0])(1e-3 if pair[0] == 'near_degenerate' else 0.3, D=pair[1])
    assert ws.NEAR_DEGENERATE_D == (4, 5, 6, 7, 8) and ws.MODE_JUMP_D == (3, 4, 5, 6, 7, 8)
