"""GPU: transform.GriffinLim / MISI (csrc/griffin_lim.hip) against the float64 restatement of
tests/oracle_griffin_lim.py and the reference's recorded outputs (tests/golden/griffin_lim.npz).

Tolerance.  The project holds one device transform to 1e-11 absolute on unit-scale signals
(tests/test_gpu_stft.py).  n iterations are 2 n transforms behind the first guess, itself a
transform: (2 n + 1) 1e-11 on x_hat, whose peak is at most 4 in every case, and the same on
X_dash relative to max |X|.  X_dash_dash, 2 n transforms, is held to the same figure relative to
its own largest bin.  The bound needs the phase projection to be well conditioned, which is
asserted on the restatement of every case: no bin of any X'' below 1e-6 of the largest, and x_hat
moving by less than 1e-12 when X moves by a relative 1e-15.

A complex64 X is compared with the restatement on the widened array: the device forms the
magnitudes in float64, numpy.abs of a complex64 array would round them to float32.
"""
import functools

import numpy as np
import pytest

import oracle_griffin_lim as og

pytestmark = pytest.mark.gpu

SINGLE = ('size64', 'size64_fading', 'size512', 'size4096', 'one_frame')


def bound(iterations):
    return (2 * iterations + 1) * 1e-11


@functools.lru_cache(maxsize=None)
def case(name):
    return og.case(name)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(og.GOLDEN) as data:
        return {key: data[key] for key in data.files}


@functools.lru_cache(maxsize=None)
def restated(name, cls, first_guess, c64=False):
    """iterations -> (x_hat, X_dash, X_dash_dash) of the restatement, conditioning asserted"""
    c = case(name)
    X = c['X'].astype(np.complex64).astype(np.complex128) if c64 else c['X']
    model = og.RESTATED[cls](X, y=c['y'], first_guess=first_guess, **c['kw'])
    states, done = {}, 0
    for iterations in og.ITERATIONS:
        for _ in range(iterations - done):
            model.step()
        done = iterations
        states[iterations] = (model.x_hat, model.X_dash, model.X_dash_dash)
    assert model.smallest > 1e-6, (name, cls, first_guess, model.smallest)
    moved = og.movement(cls, dict(c, X=X), first_guess, done)
    assert moved < 1e-12, (name, cls, first_guess, moved)
    return states


def device_class(cls):
    from pb_bss_amd import transform
    return getattr(transform, cls)


def check(model, expected, iterations, scale_X, label):
    x_hat, X_dash, X_dash_dash = expected
    errors = (np.abs(model.x_hat - x_hat).max(),
              np.abs(model.X_dash - X_dash).max() / scale_X,
              np.abs(model.X_dash_dash - X_dash_dash).max() / np.abs(X_dash_dash).max())
    print(f'{label} n={iterations}: x_hat {errors[0]:.2e} X_dash {errors[1]:.2e} '
          f'X_dash_dash {errors[2]:.2e} (bound {bound(iterations):.1e})')
    assert model.x_hat.dtype == np.float64 and model.x_hat.shape == x_hat.shape
    assert model.X_dash.dtype == np.complex128 and model.X_dash.shape == X_dash.shape
    assert model.X_dash_dash.dtype == np.complex128 and model.X_dash_dash.shape == X_dash.shape
    assert max(errors) < bound(iterations), (label, iterations, errors)


@pytest.mark.parametrize('first_guess', og.FIRST_GUESSES)
@pytest.mark.parametrize('cls', og.CLASSES)
@pytest.mark.parametrize('name', SINGLE)
def test_against_restatement_and_golden(name, cls, first_guess):
    c = case(name)
    expected = restated(name, cls, first_guess)
    assert np.abs(expected[20][0]).max() <= 4
    scale_X = np.abs(c['X']).max()
    stride = og.STRIDE.get(name, 1)
    for iterations in og.ITERATIONS:
        model = device_class(cls)(c['X'], y=c['y'], first_guess=first_guess, **c['kw'])
        assert model.X_dash is c['X'] and model.X_dash_dash is c['X']
        model.step(iterations=iterations)
        check(model, expected[iterations], iterations, scale_X, f'{name} {cls} {first_guess}')
        recorded = golden()[og.golden_key(name, cls, first_guess, iterations)]
        assert np.abs(model.x_hat[:, ::stride] - recorded).max() < bound(iterations)
    for what in ('X_dash', 'X_dash_dash') if name in og.SPECTRA else ():
        recorded = golden()[og.golden_key(name, cls, first_guess, 20, what)]
        assert np.abs(getattr(model, what) - recorded).max() < bound(20) * np.abs(recorded).max()


@pytest.mark.parametrize('cls', og.CLASSES)
@pytest.mark.parametrize('name', ['size64_fading', 'size512'])
def test_single_steps_equal_one_call_and_calls_repeat(name, cls):
    c = case(name)
    make = functools.partial(device_class(cls), c['X'], y=c['y'], first_guess='y', **c['kw'])
    stepped, at_once, again = make(), make(), make()
    for _ in range(20):
        stepped.step()
    at_once.step(iterations=20)
    again.step(iterations=20)
    for what in ('x_hat', 'X_dash', 'X_dash_dash'):
        assert np.array_equal(getattr(stepped, what), getattr(at_once, what)), what
        assert np.array_equal(getattr(again, what), getattr(at_once, what)), what
    # 5 + 15 with the estimate handed over by the caller
    resumed = make()
    resumed.step(iterations=5)
    resumed.x_hat = resumed.x_hat.copy()
    resumed.step(iterations=15)
    assert np.array_equal(resumed.x_hat, at_once.x_hat)


@pytest.mark.parametrize('cls', og.CLASSES)
@pytest.mark.parametrize('name', ['size64', 'size512'])
def test_complex64_and_device_tensors(name, cls):
    import torch
    c = case(name)
    X64 = c['X'].astype(np.complex64)
    expected = restated(name, cls, 'istft', c64=True)
    scale_X = np.abs(c['X']).max()
    host = device_class(cls)(X64, y=c['y'], first_guess='istft', **c['kw'])
    host.step(iterations=5)
    check(host, expected[5], 5, scale_X, f'{name} {cls} complex64')

    for X in (X64, c['X']):
        Xt, yt = torch.from_numpy(X).cuda(), torch.from_numpy(c['y']).cuda()
        model = device_class(cls)(Xt, y=yt, first_guess='y', **c['kw'])
        assert model.x_hat.is_cuda and model.x_hat.dtype == torch.float64
        model.step(iterations=5)
        for what, dtype in (('x_hat', torch.float64), ('X_dash', torch.complex128),
                            ('X_dash_dash', torch.complex128)):
            value = getattr(model, what)
            assert torch.is_tensor(value) and value.device == Xt.device and value.dtype == dtype
        assert model.X is Xt and model.y is yt
        same = device_class(cls)(X, y=c['y'], first_guess='y', **c['kw'])
        same.step(iterations=5)
        for what in ('x_hat', 'X_dash', 'X_dash_dash'):
            assert np.array_equal(getattr(model, what).cpu().numpy(), getattr(same, what)), what
        if X is c['X']:
            check(same, restated(name, cls, 'y')[5], 5, scale_X, f'{name} {cls} tensor')


@pytest.mark.parametrize('first_guess', og.FIRST_GUESSES)
@pytest.mark.parametrize('cls', og.CLASSES)
def test_leading_axes_equal_the_mixtures_one_by_one(cls, first_guess):
    a, b = case('batch_a'), case('batch_b')
    X, y = np.stack([a['X'], b['X']]), np.stack([a['y'], b['y']])
    assert X.shape == (2, 3, 20, 33)
    batch = device_class(cls)(X, y=y, first_guess=first_guess, **a['kw'])
    assert batch.x_hat.shape == (2, 3, y.shape[-1])
    batch.step(iterations=5)
    for index, c in enumerate((a, b)):
        single = device_class(cls)(c['X'], y=c['y'], first_guess=first_guess, **c['kw'])
        single.step(iterations=5)
        for what in ('x_hat', 'X_dash', 'X_dash_dash'):
            assert np.array_equal(getattr(batch, what)[index], getattr(single, what)), what
        name = ('batch_a', 'batch_b')[index]
        check(single, restated(name, cls, first_guess)[5], 5, np.abs(c['X']).max(),
              f'{name} {cls} {first_guess}')


@pytest.mark.parametrize('cls', og.CLASSES)
def test_zero_bins_have_the_phase_factor_one(cls):
    """numpy.angle(0) == 0: where X'' is exactly zero, X_dash is |X|.  y is zero over samples
    64..239, which frames 4..11 of 64 samples every 16 lie in; with first_guess='y' those frames
    of the first step transform zeros.  The magnitudes are 5 m with m a float32 number and
    X = m (3 + 4i) up to signs: 9 m^2 + 16 m^2 and its root are exact in float64, so that |X| is
    the same number whoever rounds the hypotenuse, and the comparison can be exact.  The
    restatement is no yardstick for these frames: numpy's rfft of an all-zero frame returns -0.0
    in the real part of one bin, numpy.angle(-0.0 + 0j) is pi, and the product is -|X| there; the
    device gives a zero bin the factor 1 whatever the sign of the zero."""
    rng = np.random.default_rng(8)
    K, T, size, shift = 3, 20, 64, 16
    n = og.samples(T, size, shift, False)
    y = rng.standard_normal(n)
    y[64:240] = 0.0
    m = rng.uniform(0.5, 2, (K, T, size // 2 + 1)).astype(np.float32).astype(np.float64)
    phasor = np.array([3 + 4j, -3 + 4j, 4 - 3j, -4 - 3j])[rng.integers(0, 4, m.shape)]
    X = m * phasor
    assert np.array_equal(np.abs(X), 5 * m)
    model = device_class(cls)(X, y=y, first_guess='y', size=size, shift=shift)
    assert np.array_equal(model.x_hat[:, 64:240], np.zeros((K, 176)))
    model.step()
    zero = slice(4, 12)
    assert np.array_equal(model.X_dash_dash[:, zero], np.zeros((K, 8, 33)))
    assert np.array_equal(model.X_dash[:, zero].real, 5 * m[:, zero])
    assert np.array_equal(model.X_dash[:, zero].imag, np.zeros((K, 8, 33)))
    assert np.isfinite(model.X_dash).all() and np.isfinite(model.x_hat).all()
    # the magnitudes are those of X everywhere, to rounding
    np.testing.assert_allclose(np.abs(model.X_dash), 5 * m, rtol=4e-15, atol=0)


def test_evaluate():
    """evaluate() against BSS-Eval of tests/oracle_bss_eval.py (1e-9 dB, the bound of
    tests/test_gpu_bss_eval.py for a Gram matrix with cond <= 1e3 and K L <= 1024) and the
    inconsistency composed from the oracle STFT on the host: mean |d|^2 with d changed by at
    most delta = 2e-11 max |X_dash| (two transforms) moves by at most 2 sqrt(mean |d|^2) delta +
    delta^2."""
    import oracle_bss_eval as ob
    from oracle import stft as ostft
    from pb_bss_amd.transform import MISI
    c = og.gen_case(77, 2, 120, 64, 16)
    assert ob.gram_condition(c['sources'], ob.FILTER_LENGTH) <= 1e3
    model = MISI(c['X'], c['y'], **c['kw'])
    model.step(iterations=5)
    got = model.evaluate(c['sources'])
    assert sorted(got) == ['inconsistency', 'mir_eval_sdr', 'mir_eval_sir']
    sdr, sir, _, _ = ob.bss_eval(c['sources'], model.x_hat)
    assert abs(got['mir_eval_sdr'] - np.mean(sdr)) < 1e-9
    assert abs(got['mir_eval_sir'] - np.mean(sir)) < 1e-9
    d = model.X_dash - ostft.stft(ostft.istft(model.X_dash, **c['kw']), **c['kw'])
    want = np.mean(d.real ** 2 + d.imag ** 2)
    delta = 2e-11 * np.abs(model.X_dash).max()
    print(f"evaluate: {got}, inconsistency on the host {want!r}")
    assert want > 1e-6
    assert abs(got['inconsistency'] - want) <= 2 * np.sqrt(want) * delta + delta ** 2

    import torch
    tensors = MISI(torch.from_numpy(c['X']).cuda(), torch.from_numpy(c['y']).cuda(), **c['kw'])
    tensors.step(iterations=5)
    on_device = tensors.evaluate(torch.from_numpy(c['sources']).cuda())
    for key, value in on_device.items():
        assert torch.is_tensor(value) and value.is_cuda and value.ndim == 0
        assert abs(float(value) - got[key]) < 1e-12, key


def test_get_variance_for_zero_mean_signal():
    """mean of re^2 + im^2 (the reference's formula); float64 sums of at most 600 positive
    terms in another order differ by a few 1e-16 relative"""
    import torch
    from pb_bss_amd.evaluation.sxr_module import get_variance_for_zero_mean_signal as variance
    rng = np.random.default_rng(9)
    real = rng.standard_normal((3, 4, 50))
    cplx = rng.standard_normal((3, 4, 50)) + 1j * rng.standard_normal((3, 4, 50))
    for x in (real, cplx, cplx.astype(np.complex64), real.astype(np.float32)):
        wide = x.astype(np.complex128)
        for axis in (None, -1, 0, (0, 2)):
            for keepdims in (False, True):
                want = np.mean(wide.real ** 2 + wide.imag ** 2, axis=axis, keepdims=keepdims)
                got = variance(x, axis=axis, keepdims=keepdims)
                assert np.shape(got) == np.shape(want) and got.dtype == np.float64
                np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
        tensor = variance(torch.from_numpy(x).cuda(), axis=-1)
        assert tensor.is_cuda and tensor.dtype == torch.float64
        assert np.array_equal(tensor.cpu().numpy(), variance(x, axis=-1))
    assert np.ndim(variance(cplx)) == 0


def test_first_guess_noise_and_limits():
    from pb_bss_amd.transform import GriffinLim, MISI
    c = case('one_frame')
    np.random.seed(3)
    model = GriffinLim(c['X'], first_guess='white_gaussian_noise', **c['kw'])
    np.random.seed(3)
    assert np.array_equal(model.x_hat, np.random.randn(2, c['y'].shape[-1]))
    model.step(iterations=2)
    assert model.x_hat.shape == (2, c['y'].shape[-1]) and np.isfinite(model.x_hat).all()
    np.testing.assert_allclose(np.abs(model.X_dash), np.abs(c['X']), rtol=1e-14)
    with pytest.raises(ValueError):
        model.step(iterations=0)
    # Griffin-Lim ignores y unless the first guess is made of it
    ignored = GriffinLim(c['X'], y=c['y'][:-3], **c['kw'])
    ignored.step()
    plain = GriffinLim(c['X'], **c['kw'])
    plain.step()
    assert np.array_equal(ignored.x_hat, plain.x_hat)
    # nine sources: Griffin-Lim serves them, MISI holds at most eight sums per thread
    X9 = np.concatenate([c['X']] * 5)[:9]
    GriffinLim(X9, **c['kw']).step()
    with pytest.raises(NotImplementedError):
        MISI(X9, c['y'], **c['kw']).step()
    eight = MISI(X9[:8], c['y'], **c['kw'])
    eight.step(iterations=2)
    want = og.run(og.MISI, X9[:8], c['y'], 'istft', 2, **c['kw'])
    assert want.smallest > 1e-6
    assert np.abs(eight.x_hat - want.x_hat).max() < bound(2)
