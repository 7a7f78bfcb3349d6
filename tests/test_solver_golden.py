"""The multiprecision fixture of the hard solver cases (tests/golden/solver_hard_cases.npz, recipe
oracle/make_solver_golden.py) is complete, consistent, and a yardstick LAPACK itself meets.

No GPU: tests/test_gpu_solvers_hard.py holds the device against the same fixture, the same
metrics (oracle/solver_cases.py) and the same first-order floors."""
import os

import numpy as np
import pytest

from oracle import solver_cases as sc

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'solver_hard_cases.npz')


@pytest.fixture(scope='module')
def fx():
    return sc.load_fixture(PATH)


@pytest.fixture(scope='module')
def cases(fx):
    return sc.fixture_cases(fx)


def _keys(fx, solver):
    return sorted({k.rsplit('|', 1)[0] for k in fx if k.startswith(solver + '|')},
                  key=lambda k: (int(k.split('|')[2]), k))


def test_fixture_is_small():
    assert os.path.getsize(PATH) < 300 * 1024


def test_no_family_or_size_is_missing(fx):
    """A regenerated fixture cannot silently shrink: every family at every size of the issue."""
    missing = []

    def need(key, fields):
        for f in fields:
            try:
                sc.ref(fx, key, f)
            except KeyError:
                missing.append(f'{key}|{f}')

    assert sc.SIZES == (2, 3, 4, 5, 6, 7, 8, 9, 17, 32, 34)
    # literally, not from the generator's own constants: lowering one must fail here
    assert (sc.PENCIL_MAX_D, sc.BEAMFORMER_MAX_D, sc.LCMV_MAX_D) == (32, 32, 8)
    small_heev = {'graded_k1e4', 'graded_k1e8', 'graded_k1e12', 'graded_k1e16', 'cluster',
                  'indefinite', 'rank1', 'rankDm1', 'neardiag', 'eqdiag', 'realsym', 'imagoff',
                  'scaled_p80', 'scaled_m80', 'scaled_p250', 'scaled_m250'}
    for D in sc.SIZES:
        fams = set(sc.heev_families(D))
        assert fams == (small_heev if D < 17 else small_heev - {
            'graded_k1e4', 'graded_k1e12', 'graded_k1e16', 'rankDm1'})
        for fam in fams:
            need(f'heev|{fam}|{D}', ('w', 'v', 'info', 'lapack'))
        if D > 32:  # the generic solve / gev kernels stop there
            continue
        sfams = set(sc.solve_families(D))
        assert sfams == ({'k1e2', 'k1e8', 'k1e12', 'scaled_p80', 'scaled_m80'} if D < 17 else
                         {'k1e8', 'scaled_p80', 'scaled_m80'})
        for fam in sfams:
            need(f'solve|{fam}|{D}', ('x', 'info', 'lapack'))
        gfams = set(sc.gev_families(D))
        assert gfams == ({'noise_k1e2', 'noise_k1e6', 'noise_k1e10', 'scaled_40'} if D < 17 else
                         {'noise_k1e6', 'scaled_40'})
        for fam in gfams:
            fields = ['w', 'lam', 'info', 'lapack', 'lapack_eig']
            fields += ['mvdr', 'souden_mat', 'souden_num', 'souden_den', 'wmwf_mat', 'ban',
                       'bf_lapack']
            if D <= 8:  # pbbss_lcmv's limit
                fields.append('lcmv')
            need(f'gev|{fam}|{D}', fields)
        need(f'gevgen|nonherm|{D}', ('w', 'lam', 'info', 'lapack_eig'))
    assert not missing, missing
    # M in {1, 2, D} right-hand sides
    assert {sc.ref(fx, f'solve|{f}|5', 'x').shape[1] for f in ('k1e2', 'k1e8', 'k1e12')} == {1, 2, 5}


def test_inputs_are_as_declared(fx, cases):
    for key in _keys(fx, 'heev'):
        a = sc.inputs(cases, key)['a']
        D = int(key.split('|')[2])
        assert a.shape == (D, D) and np.isfinite(a).all(), key
        assert np.array_equal(a, a.conj().T), key
        fam = key.split('|')[1]
        if fam == 'realsym':
            assert not a.imag.any(), key
        if fam == 'imagoff':
            assert not (a.real - np.diag(np.diag(a.real))).any(), key
        if fam == 'eqdiag':
            assert (np.diag(a) == 0.5).all(), key
        w, info = sc.ref(fx, key, 'w'), sc.ref(fx, key, 'info')
        assert (np.diff(w) >= 0).all() and info[0] == max(abs(w[0]), abs(w[-1])), key
    for key in _keys(fx, 'gev'):
        x = sc.inputs(cases, key)
        for m in (x['t'], x['n']):
            assert np.isfinite(m).all() and np.array_equal(m, m.conj().T), key
        assert np.linalg.eigvalsh(x['n'])[0] > 0, key
    for key in _keys(fx, 'solve') + _keys(fx, 'gevgen'):
        assert all(np.isfinite(v).all() for v in sc.inputs(cases, key).values()), key
    for key in _keys(fx, 'gevgen'):  # the target really is non-Hermitian
        t = sc.inputs(cases, key)['t']
        assert not np.allclose(t, t.conj().T), key


def test_scaled_cases_scale_exactly(fx, cases):
    """Power-of-two scaling: inputs and reference eigenvalues are exact multiples."""
    for D in sc.SIZES:
        base = sc.inputs(cases, f'heev|{sc.HEEV_BASE}|{D}')['a']
        for fam, s in (('scaled_p80', 80), ('scaled_m80', -80), ('scaled_p250', 250),
                       ('scaled_m250', -250)):
            assert np.array_equal(sc.inputs(cases, f'heev|{fam}|{D}')['a'], base * 2.0 ** s)
            assert np.array_equal(sc.ref(fx, f'heev|{fam}|{D}', 'w'),
                                  sc.ref(fx, f'heev|{sc.HEEV_BASE}|{D}', 'w') * 2.0 ** s)


def _worst(table, name, ratio, key):
    if ratio > table.get(name, (0.0, ''))[0]:
        table[name] = (ratio, key)


def test_lapack_stays_within_the_floors(fx, cases):
    """LAPACK, re-measured now against the stored multiprecision references, meets every
    first-order floor that the device is held to (there with a factor of 16 on top).

    Two metrics of eigh are the exception: its residual and its orthogonality defect sit near
    7 eps at every size, which is above D eps for small D (worst here: orthogonality
    1.36 D eps, eqdiag D = 4; residual 1.15 D eps, indefinite D = 6).  They are held to 2 floors."""
    import scipy.linalg
    worst = {}
    for key in _keys(fx, 'heev'):
        D = int(key.split('|')[2])
        a = sc.inputs(cases, key)['a']
        w, V = np.linalg.eigh(a)
        m = sc.heev_metrics(a, w, V, sc.ref(fx, key, 'w'), sc.ref(fx, key, 'v'))
        fl = sc.heev_floors(D, sc.ref(fx, key, 'info'))
        cluster = key.split('|')[1] == 'cluster'
        for i, name in enumerate(('val', 'res', 'orth', 'ang', 'proj')):
            if (name == 'ang' and cluster) or (name == 'proj' and not cluster):
                continue  # the principal vector of a cluster is ill-defined; its plane is not
            _worst(worst, 'heev ' + name, m[i] / fl[i], key)
    for key in _keys(fx, 'solve'):
        D = int(key.split('|')[2])
        x = sc.inputs(cases, key)
        err = sc.rel_fro(np.linalg.solve(x['a'], x['b']), sc.ref(fx, key, 'x'))
        _worst(worst, 'solve', err / sc.solve_floor(D, sc.ref(fx, key, 'info')), key)
    for key in _keys(fx, 'gev'):
        D = int(key.split('|')[2])
        x = sc.inputs(cases, key)
        fl = sc.gev_floors(D, sc.ref(fx, key, 'info'))
        _, V = scipy.linalg.eigh(x['t'], x['n'])
        m = sc.gev_metrics(x['t'], x['n'], V[:, -1], sc.ref(fx, key, 'w'), sc.ref(fx, key, 'lam'))
        for i, name in enumerate(('lam', 'ang', 'norm')):
            _worst(worst, 'gev ' + name, m[i] / fl[i], key)
        f64 = sc.beamformers_f64(x['t'], x['n'], x['atf'], x['atf2'], sc.ref(fx, key, 'w'))
        for f, v in f64.items():
            _worst(worst, f, sc.rel_fro(v, sc.ref(fx, key, f)) / fl[0], key)
    for key in _keys(fx, 'gev') + _keys(fx, 'gevgen'):
        D = int(key.split('|')[2])
        x = sc.inputs(cases, key)
        fl = sc.gev_floors(D, sc.ref(fx, key, 'info'))
        le, Ve = scipy.linalg.eig(x['t'], x['n'])
        k = int(np.argmax(le))
        m = sc.gev_metrics(x['t'], x['n'], Ve[:, k], sc.ref(fx, key, 'w'), sc.ref(fx, key, 'lam'),
                           le[k])
        for i, name in ((0, 'lam'), (1, 'ang'), (3, 'ret')):
            _worst(worst, 'eig ' + name, m[i] / fl[i], key)
    for name, (ratio, key) in sorted(worst.items()):
        print(f'{name:12s} worst error / floor = {ratio:9.3g}   {key}')
    bad = {n: v for n, v in worst.items()
           if not v[0] <= (2.0 if n in ('heev res', 'heev orth') else 1.0)}
    assert not bad, bad


def test_recipe_reproduces_three_cases(fx, cases):
    """Where mpmath is installed: one heev, one gev and one solve case at D = 5, re-derived in 50
    digits, agree with the fixture to 1e-15."""
    pytest.importorskip('mpmath')
    from oracle import make_solver_golden as recipe

    def close(got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert np.max(np.abs(got - want)) <= 1e-15 * np.max(np.abs(want))

    built = sc.build_cases()
    for key in ('heev|graded_k1e8|5', 'gev|noise_k1e6|5', 'solve|k1e8|5'):
        for f, v in built[key].items():  # the seeded generator gives the stored inputs
            assert np.array_equal(v, cases[key][f]), (key, f)
    w, v, info = recipe.mp_heev(sc.inputs(cases, 'heev|graded_k1e8|5')['a'])
    close(w, fx['heev|graded_k1e8|5|w'])
    close(v[:, :1], fx['heev|graded_k1e8|5|v'])
    close(info, fx['heev|graded_k1e8|5|info'])
    x = sc.inputs(cases, 'gev|noise_k1e6|5')
    gw, lam, info = recipe.mp_gev(x['t'], x['n'])
    close(gw, fx['gev|noise_k1e6|5|w'])
    close(lam, fx['gev|noise_k1e6|5|lam'])
    x = sc.inputs(cases, 'solve|k1e8|5')
    sx, info = recipe.mp_solve(x['a'], x['b'])
    close(sx, fx['solve|k1e8|5|x'])
    close(info, fx['solve|k1e8|5|info'])
