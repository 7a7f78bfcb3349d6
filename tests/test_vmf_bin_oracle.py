"""CPU: the inputs of tests/test_gpu_vmf_bin.py do what they promise, and the oracle they are
compared with is as accurate as the GPU tolerances presuppose.

tests/oracle_vmf_bin.py chooses noise levels so that a class's raw concentration lands above the
cap, below the floor or between them; whether it does is a property of the drawn rows, so it is
asserted here from the ORACLE alone (unclipped oracle.embed.vmf_fit), with a margin of 3 % that no
rounding of a device sum can cross.  The figures are printed (pytest -s).
"""
import numpy as np
import pytest

import oracle_vmf_bin as vb
from oracle import embed as oe

MARGIN = 1.03
ALL = [(name, param) for name, lst in vb.CASES.items() for param, _ in lst]


def check_promises(c):
    """Every raw concentration is on its promised side of the clamps, 3 % away at least."""
    for k, promise in enumerate(c['promise']):
        raw = c['raw'][:, k]
        assert np.isfinite(raw).all() and (raw > 0).all(), (k, raw)
        if promise == 'high':
            assert (raw >= c['cmax'] * MARGIN).all(), (k, raw.min(), c['cmax'])
        elif promise == 'low':
            assert (raw <= c['cmin'] / MARGIN).all(), (k, raw.max(), c['cmin'])
        else:
            assert promise == 'free', promise
            assert (raw >= c['cmin'] * MARGIN).all(), (k, raw.min(), c['cmin'])
            assert (raw <= c['cmax'] / MARGIN).all(), (k, raw.max(), c['cmax'])


@pytest.mark.parametrize('E', vb.E_LIST)
@pytest.mark.parametrize('name,param', ALL)
def test_scenario_meets_its_conditions(name, param, E):
    for dtype in ('float32', 'float64'):
        c = vb.case(name, param, E, dtype)
        assert c['y'].shape == (vb.B, c['N'] + c['P'], E) and c['y'].dtype == np.dtype(dtype)
        check_promises(c)
        conc = c['model']['concentration']
        for k, promise in enumerate(c['promise']):  # the oracle's own model sits on the clamp
            if promise == 'high':
                assert (conc[:, k] == c['cmax']).all()
            elif promise == 'low':
                assert (conc[:, k] == c['cmin']).all()
            else:  # (probes appended: the sums run over other blocks, not bit-identical)
                np.testing.assert_allclose(conc[:, k], c['raw'][:, k], rtol=1e-12)
        # probes: saliency 0, unit rows, posterior of class 0 where it can still move
        P = c['P']
        assert (c['saliency'][:, -P:] == 0).all() and (c['saliency'][:, :-P] >= 0.1).all()
        assert np.abs(np.linalg.norm(c['y'][:, -P:].astype(np.float64), axis=-1) - 1).max() < 1e-6
        p = c['affiliation'][:, 0, -P:]
        inside = ((p >= 0.05) & (p <= 0.95)).mean()
        sums = (c['init'] * c['saliency'][:, None, :]).sum(-1)
        print(f'{name} {param} E={E} {dtype}: raw kappa ' +
              ' / '.join(f"{c['raw'][:, k].min():.4g}..{c['raw'][:, k].max():.4g}"
                         for k in range(c['K'])) +
              f' | probes inside {inside:.3f} ({p.min():.3f}..{p.max():.3f})')
        assert inside >= 0.9, inside
        assert (sums > 0).all()
        if 'target' in dict(vb.CASES[name])[param]:
            assert np.abs(c['raw'][:, 0] / param - 1).max() < 1e-3


def test_a_concentration_within_three_percent_of_a_clamp_is_refused():
    """The margin has teeth: the same rows with the cap moved to 2 % above / below the raw
    concentration of a class fail check_promises."""
    c = dict(vb.case('unclamped_upper_table', 900, 12))
    check_promises(c)
    for cmax in (c['raw'][:, 0].max() * 1.02, c['raw'][:, 0].min() / 1.02):
        with pytest.raises(AssertionError):
            check_promises(dict(c, cmax=cmax))
    c = dict(vb.case('clamped_low', 5, 12))
    with pytest.raises(AssertionError):
        check_promises(dict(c, cmin=c['raw'][:, 1].max() * 1.02))
    with pytest.raises(AssertionError):   # and a class on the wrong side altogether
        check_promises(dict(c, promise=('free', 'free')))


def test_hard_initialisation_is_what_lets_a_tight_class_reach_the_cap():
    """With one-hot labels a class of noise 0.01 has a raw concentration near 1 / sigma^2 = 1e4;
    with soft 0.9 / 0.1 labels a tenth of the OTHER class's spread rows caps it near 50 -- no
    clamp at 80 or above would ever bind."""
    for E in (2, 12):
        y, init, sal = vb.scenario(E, 2, vb.N_ROWS, (0.01, 0.8), 7, np.float64)
        hard = vb.raw_concentration(y, init, sal)[:, 0]
        soft = vb.raw_concentration(y, 0.8 * init + 0.1, sal)[:, 0]
        print(f'E={E}: hard {hard.min():.4g}..{hard.max():.4g}, soft {soft.min():.3g}..{soft.max():.3g}')
        assert (hard > 5e3).all() and (soft < 80).all()


def test_probes_do_not_change_the_m_step_and_sit_between_the_crossings():
    y, init, sal = vb.scenario(8, 2, 120, (0.05, 0.8), 3, np.float64)
    model, _ = vb.fit_reference(y, init, sal, 1, 1e-10, 500.0)
    yp, ip, sp = vb.with_probes(y, init, sal, model, 32)
    assert yp.shape == (vb.B, 152, 8) and ip.shape == (vb.B, 2, 152) and sp.shape == (vb.B, 152)
    assert np.array_equal(yp[:, :120], y) and (sp[:, 120:] == 0).all()
    again, aff = vb.fit_reference(yp, ip, sp, 1, 1e-10, 500.0)
    for key in ('mean', 'concentration', 'weight'):
        np.testing.assert_allclose(again[key], model[key], rtol=1e-13, atol=1e-15)
    p = aff[:, 0, 120:]
    assert (p > 0.05).all() and (p < 0.95).all()
    assert (np.diff(p, axis=-1) < 0).all()   # class 0 loses the row on the way to mean 1
    # what the probes are for: an error delta of the offset difference moves them by
    # gamma (1 - gamma) delta >= 0.0475 delta
    assert (p * (1 - p)).min() >= 0.0475 - 1e-12


KAPPAS = (1e-10, 1e-6, 1e-3, 0.5, 7.9, 80, 499, 500, 528, 529, 960, 961, 976, 977, 2000, 1e4)
DIMS = (1, 2, 3, 4, 7, 8, 12, 13, 16, 40)


def test_oracle_log_norm_against_60_digit_bessel():
    """oracle.embed.vmf_log_norm (scipy's scaled ive) against mpmath.besseli at 60 digits: what the
    GPU tolerances can blame on the reference.  Measured: 5.1e-15 relative at worst."""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 60
    worst = 0.0
    for d in DIMS:
        nu = mp.mpf(d) / 2 - 1
        for kappa in KAPPAS:
            x = mp.mpf(kappa)
            want = mp.mpf(d) / 2 * mp.log(2 * mp.pi) + mp.log(mp.besseli(nu, x)) - nu * mp.log(x)
            got = float(oe.vmf_log_norm(np.float64(kappa), d))
            err = abs(float((mp.mpf(got) - want) / want))
            worst = max(worst, err)
            assert err <= 1e-13, (d, kappa, got, float(want), err)
    print(f'vmf_log_norm against mpmath: worst relative error {worst:.1e}')
