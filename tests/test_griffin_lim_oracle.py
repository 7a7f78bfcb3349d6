"""CPU: the restatement of Griffin-Lim and MISI (tests/oracle_griffin_lim.py) against the live
reference and the golden file, the public names of `pb_bss_amd.transform`, and the argument
errors, which are raised before anything touches the device."""
import inspect

import numpy as np
import pytest

import oracle_griffin_lim as og


@pytest.fixture(scope='module')
def golden():
    with np.load(og.GOLDEN) as data:
        return {key: data[key] for key in data.files}


@pytest.mark.needs_reference
@pytest.mark.parametrize('fading', [False, True])
def test_restatement_matches_live_reference(fading):
    reference = dict(zip(og.CLASSES, og.load_reference()))
    fresh = og.gen_case(1234 + fading, 2, 9, 128, 32, fading)
    for cls in og.CLASSES:
        for first_guess in og.FIRST_GUESSES:
            ref = reference[cls](fresh['X'], y=fresh['y'], first_guess=first_guess, **fresh['kw'])
            own = og.RESTATED[cls](fresh['X'], y=fresh['y'], first_guess=first_guess,
                                   **fresh['kw'])
            np.testing.assert_allclose(own.x_hat, ref.x_hat, rtol=0, atol=1e-13)
            for _ in range(7):
                ref.step()
                own.step()
                for what in ('x_hat', 'X_dash', 'X_dash_dash'):
                    np.testing.assert_allclose(getattr(own, what), getattr(ref, what), rtol=0,
                                               atol=1e-13, err_msg=f'{cls} {first_guess} {what}')


@pytest.mark.parametrize('name', og.RECORDED)
def test_restatement_matches_golden(golden, name):
    entries = og.golden_entries(og.RESTATED, name)
    assert entries and set(entries) <= set(golden)
    for key, value in entries.items():
        assert value.shape == golden[key].shape, key
        np.testing.assert_allclose(value, golden[key], rtol=0, atol=1e-13, err_msg=key)


def test_golden_holds_the_recorded_cases_only(golden):
    expected = set()
    for name in og.RECORDED:
        expected |= set(og.golden_entries(og.RESTATED, name))
    assert set(golden) == expected


@pytest.mark.parametrize('name', list(og.CASES))
def test_cases_are_well_conditioned(name):
    """what the device tolerance rests on: no bin of any X'' near zero, and x_hat insensitive to
    the last bits of X"""
    case = og.case(name)
    assert 1 <= np.abs(case['y']).max() <= 5
    for cls in og.CLASSES:
        for first_guess in og.FIRST_GUESSES:
            model = og.run(og.RESTATED[cls], case['X'], case['y'], first_guess, 20, **case['kw'])
            assert model.smallest > 1e-6, (cls, first_guess, model.smallest)
            assert og.movement(cls, case, first_guess, 20) < 1e-12, (cls, first_guess)


def test_public_names():
    from pb_bss_amd import transform
    from pb_bss_amd.transform import griffin_lim_module
    assert 'GriffinLim' in transform.__all__ and 'MISI' in transform.__all__
    assert transform.GriffinLim is griffin_lim_module.GriffinLim
    assert transform.MISI is griffin_lim_module.MISI
    assert issubclass(transform.MISI, transform.GriffinLim)
    parameters = inspect.signature(transform.GriffinLim.__init__).parameters
    assert list(parameters) == ['self', 'X', 'y', 'first_guess', 'size', 'shift', 'fading']
    defaults = {name: p.default for name, p in parameters.items() if name not in ('self', 'X')}
    assert defaults == dict(y=None, first_guess='istft', size=512, shift=128, fading=False)
    assert inspect.signature(transform.MISI.__init__) == inspect.signature(
        transform.GriffinLim.__init__)
    assert list(inspect.signature(transform.GriffinLim.step).parameters) == ['self', 'iterations']
    for cls in (transform.GriffinLim, transform.MISI):
        assert inspect.signature(cls.step).parameters['iterations'].default == 1
    from pb_bss_amd.evaluation import sxr_module
    assert callable(sxr_module.get_variance_for_zero_mean_signal)
    assert 'get_variance_for_zero_mean_signal' not in sxr_module.__all__


@pytest.mark.needs_reference
def test_constructor_parameters_are_the_reference_s():
    from pb_bss_amd import transform
    for own, ref in zip((transform.GriffinLim, transform.MISI), og.load_reference()):
        mine = inspect.signature(own.__init__).parameters
        theirs = inspect.signature(ref.__init__).parameters
        assert list(mine) == list(theirs)
        assert [p.default for p in mine.values()] == [p.default for p in theirs.values()]


def test_argument_errors(monkeypatch):
    """Every one of these is raised before a device call: none of them may reach the library."""
    from pb_bss_amd import _lib
    from pb_bss_amd.transform import GriffinLim, MISI

    def no_device(*args, **kwargs):
        raise AssertionError('an argument error has to be raised before any device call')

    for name in ('load', 'handle', 'launch', 'require_gpu', 'to_device'):
        monkeypatch.setattr(_lib, name, no_device)

    case = og.case('one_frame')
    X, y, kw = case['X'], case['y'], case['kw']
    for cls in (GriffinLim, MISI):
        with pytest.raises(ValueError, match='^nonsense$'):
            cls(X, y, first_guess='nonsense', **kw)
        with pytest.raises(ValueError):
            cls(X, y[:-1], first_guess='y', **kw)
        with pytest.raises(ValueError):
            cls(X, np.concatenate([y, y[:16]]), first_guess='y', **kw)   # one frame more
        with pytest.raises(ValueError):
            cls(X[0], y, **kw)                                           # no source axis
        with pytest.raises(ValueError):
            cls(X, y, size=128, shift=32)                                # F is not size // 2 + 1
        with pytest.raises(ValueError):
            cls(X[..., :49], y, size=96, shift=16)                       # no power of two
        with pytest.raises(ValueError):
            cls(X, y, size=64, shift=24)                                 # size % shift
        with pytest.raises(TypeError):
            cls(X, None, first_guess='y', **kw)
    with pytest.raises((TypeError, ValueError)):
        MISI(X, **kw)
    with pytest.raises((TypeError, ValueError)):
        MISI(X, None, first_guess='white_gaussian_noise', **kw)
    with pytest.raises(ValueError):
        MISI(X, y[:-1], **kw)
    with pytest.raises(ValueError):
        MISI(X, np.stack([y, y]), **kw)                                  # a batch of y, one of X
    with pytest.raises(ValueError):
        MISI(np.stack([X, X]), y, **kw)
