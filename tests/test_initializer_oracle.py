"""CPU: the deflation-seed restatement (tests/oracle_initializer.py) against the reference's
recorded results and the live reference; the i.i.d. / flag initialisers in 'numpy' mode against
the reference's recorded doctest arrays; the import surface of pb_bss_amd.initializer."""
import glob
import os

import numpy as np
import pytest

import oracle_initializer as oi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEFLATION = sorted(glob.glob(os.path.join(GOLDEN, 'initializer_deflation_*.npz')))
# restatement vs reference: reordered float64 sums only (measured 2e-15 .. 1.3e-13)
RESTATEMENT_TOL = 1e-12


def test_import_surface():
    import pb_bss_amd.initializer as init
    from pb_bss_amd import _lib
    from pb_bss_amd.initializer import deflation, deterministic, iid
    assert init.iid is iid and init.deflation is deflation and init.deterministic is deterministic
    assert iid.__all__ == ['uniform_normalized', 'dirichlet_uniform', 'dirichlet', 'one_hot']
    for name in iid.__all__:
        assert callable(getattr(iid, name))
    assert callable(deflation.deflationSeed) and callable(deterministic.flag)
    assert 'pbbss_deflation_seed' in _lib.EXPORTS
    assert hasattr(_lib.load(), 'pbbss_deflation_seed')
    import inspect
    sig = inspect.signature(deflation.deflationSeed)
    assert list(sig.parameters) == ['Y', 'sources', 'saliencies', 'permutation_free', 'neighbors',
                                    'similarity_transform', 'eps']
    assert sig.parameters['permutation_free'].default is True
    assert sig.parameters['neighbors'].default == 5 and sig.parameters['eps'].default == 0
    assert inspect.signature(deterministic.flag).parameters['minimum'].default == 0
    assert inspect.signature(iid.dirichlet).parameters['alpha'].default == 1


@pytest.mark.needs_reference
def test_import_surface_matches_reference():
    from oracle import refshim
    refshim.load()
    import inspect

    import pb_bss.initializer as ref
    import pb_bss_amd.initializer as init
    assert init.iid.__all__ == ref.iid.__all__
    pairs = [(getattr(init.iid, n), getattr(ref.iid, n)) for n in ref.iid.__all__]
    pairs += [(init.deflation.deflationSeed, ref.deflation.deflationSeed),
              (init.deterministic.flag, ref.deterministic.flag)]
    for mine, theirs in pairs:
        a, b = inspect.signature(mine), inspect.signature(theirs)
        assert list(a.parameters) == list(b.parameters), mine.__name__
        for name in a.parameters:
            assert a.parameters[name].default == b.parameters[name].default, (mine.__name__, name)


def test_fixtures_present():
    assert len(DEFLATION) == 4, DEFLATION
    for path in DEFLATION + [os.path.join(GOLDEN, 'initializer_iid.npz')]:
        assert os.path.getsize(path) < 1024 * 1024, path


@pytest.mark.parametrize('path', DEFLATION, ids=[os.path.basename(p)[:-4] for p in DEFLATION])
@pytest.mark.parametrize('pf', [True, False])
def test_restatement_matches_recorded_reference(path, pf):
    g = np.load(path)
    F, T, D, K, seed, nb = (int(g[k]) for k in ('F', 'T', 'D', 'K', 'seed', 'neighbors'))
    Y = oi.synth_case(F, T, D, K, seed)
    details = {}
    post = oi.deflation_seed(Y, K, permutation_free=pf, neighbors=nb, details=details)
    oi.assert_well_determined(details)
    ref = g[f'posterior_pf{int(pf)}']
    assert post.shape == ref.shape == (K, F, T)
    err = float(np.abs(post - ref).max())
    print(f'{os.path.basename(path)} pf={pf}: restatement vs reference {err:.2e}, '
          f'argmax gaps {details["argmax_gap"]}, eig gaps {details["eig_gap"]}')
    assert err <= RESTATEMENT_TOL, err
    # the silenced bin and the zero-padded frames belong to the last class, exactly
    expect = np.zeros(K)
    expect[-1] = 1
    assert (ref[:, 3, :] == expect[:, None]).all() and (post[:, 3, :] == expect[:, None]).all()
    if T >= 64:
        assert (post[:, :, T - 10:] == expect[:, None, None]).all()
    if pf:
        assert (details['peaks'] == details['peaks'][:, :1]).all()


@pytest.mark.needs_reference
@pytest.mark.parametrize('pf', [True, False])
def test_restatement_matches_live_reference(pf):
    from oracle import refshim
    refshim.load()
    from pb_bss.initializer import deflation
    rng = np.random.default_rng(5)

    def soften(similarity, saliencies):
        return similarity ** 2 * (saliencies >= 0)

    for seed, (F, T, D, K, nb) in enumerate([(257, 50, 3, 3, 5), (257, 70, 5, 4, 2),
                                             (513, 30, 7, 2, 4)], start=40):
        Y = oi.synth_case(F, T, D, K, seed).astype(np.complex128)
        given = rng.uniform(0.1, 1.0, size=(F, T)) * np.linalg.norm(Y, axis=-1)
        for kw in (dict(), dict(saliencies=given), dict(similarity_transform=soften),
                   dict(eps=1e-3), dict(saliencies=given, eps=1e-2, similarity_transform=soften)):
            ref = np.asarray(deflation.deflationSeed(Y, K, permutation_free=pf, neighbors=nb, **kw))
            details = {}
            mine = oi.deflation_seed(Y, K, permutation_free=pf, neighbors=nb, details=details, **kw)
            oi.assert_well_determined(details)
            err = float(np.abs(mine - ref).max())
            print(f'F={F} T={T} D={D} K={K} pf={pf} {sorted(kw)}: {err:.2e}')
            assert err <= RESTATEMENT_TOL, (sorted(kw), err)


def test_iid_and_flag_numpy_mode_match_recorded_reference():
    """'numpy' mode consumes NumPy's global stream call for call like the reference: the
    reference's doctest arrays come back bit for bit.  NumPy input: no GPU involved."""
    from pb_bss_amd.distribution.utils import random_init
    from pb_bss_amd.initializer import deterministic, iid
    g = np.load(os.path.join(GOLDEN, 'initializer_iid.npz'))
    ones = np.ones([4, 5, 3])
    with random_init('numpy'):
        for name in iid.__all__:
            np.random.seed(0)
            a = getattr(iid, name)(ones, 2)
            b = getattr(iid, name)(ones, 2, permutation_free=True)
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (4, 2, 5)
            assert np.array_equal(a, g[f'{name}_pf0']), name
            assert np.array_equal(b, g[f'{name}_pf1']), name
            assert np.array_equal(b[0], b[3])
    assert np.array_equal(deterministic.flag(ones, 2, permutation_free=True), g['flag_4_2'])
    assert np.array_equal(
        deterministic.flag(np.ones([1, 5, 3]), 2, minimum=0.1, permutation_free=True),
        g['flag_1_2_min'])
    assert np.array_equal(
        deterministic.flag(np.ones([1, 5, 3]), 4, minimum=0.1, permutation_free=True),
        g['flag_1_4_min'])
    with pytest.raises(NotImplementedError):
        deterministic.flag(ones, 2)
    with pytest.raises(AssertionError):
        deterministic.flag(ones, 2, permutation_free=True, minimum=0.5)


def test_iid_properties_numpy_mode():
    from pb_bss_amd.initializer import iid
    Y = np.ones([3, 2, 17, 4])
    np.random.seed(3)
    for name in iid.__all__:
        for pf in (False, True):
            a = getattr(iid, name)(Y, 5, permutation_free=pf)
            assert a.shape == (3, 2, 5, 17)
            assert np.allclose(a.sum(-2), 1, rtol=0, atol=1e-14) and (a >= 0).all()
            if pf:
                assert np.array_equal(a, np.broadcast_to(a[0, 0], a.shape))
    hot = iid.one_hot(Y, 5)
    assert set(np.unique(hot)) == {0.0, 1.0}
