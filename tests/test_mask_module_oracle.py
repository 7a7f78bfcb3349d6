"""CPU: the import surface of pb_bss_amd.extraction.mask_module, the float64 restatement of the
oracle masks (tests/oracle_masks.py) against the reference's recorded results
(tests/golden/mask_module_*.npz) and against the live reference, and
voiced_unvoiced_split_characteristic bit for bit."""
import inspect
import os

import numpy as np
import pytest

import oracle_masks as om

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# restatement vs reference: the same float64 operations, at most a reordered sum or an
# algebraically equal form (ratio masks); values of order one
TOL = 1e-13


def golden(name):
    return np.load(os.path.join(GOLDEN, f'mask_module_{name}.npz'))


def biased_input(shape):
    x = om.gen(2, shape).astype(np.complex128)
    x[1] *= 0.3
    return x


def test_import_surface():
    from pb_bss_amd import _lib, extraction
    from pb_bss_amd.extraction import mask_module
    assert mask_module.__all__ == om.NAMES
    for name in om.NAMES:
        assert callable(getattr(mask_module, name)), name
        assert getattr(extraction, name) is getattr(mask_module, name), name
        assert name in extraction.__all__, name
    assert len(set(extraction.__all__)) == len(extraction.__all__)
    from pb_bss_amd.extraction import wiener_like_mask  # noqa: F401
    for export in ('pbbss_mask_pointwise', 'pbbss_mask_lorenz', 'pbbss_mask_quantile'):
        assert export in _lib.EXPORTS and hasattr(_lib.load(), export)
    sig = inspect.signature(mask_module.lorenz_mask)
    assert list(sig.parameters) == ['signal', 'sensor_axis', 'axis', 'lorenz_fraction', 'weight',
                                    'keepdims']
    assert all(p.kind is p.KEYWORD_ONLY for n, p in sig.parameters.items() if n != 'signal')
    assert sig.parameters['axis'].default == (-2, -1)
    assert sig.parameters['lorenz_fraction'].default == 0.98
    sig = inspect.signature(mask_module.quantile_mask)
    assert sig.parameters['quantile'].default == (0.1, -0.9)
    assert sig.parameters['axis'].default == -2 and sig.parameters['axis'].kind is \
        inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(mask_module.wiener_like_mask).parameters['eps'].default == 1e-18
    assert inspect.signature(mask_module.biased_binary_mask).parameters['high_cut'].default == 500


def test_mask_geom_struct_layout():
    import ctypes
    from pb_bss_amd import _lib
    # 3 x 4 int64, 4 int64, 2 int32: 136 bytes, like the C struct
    assert ctypes.sizeof(_lib.MaskGeom) == 136
    assert _lib.MaskGeom.x_source_stride.offset == 96
    assert _lib.MaskGeom.sources.offset == 128


@pytest.mark.needs_reference
def test_signatures_match_reference():
    from oracle import refshim
    refshim.load()
    from pb_bss.extraction import mask_module as ref
    from pb_bss_amd.extraction import mask_module
    assert mask_module.__all__ == ref.__all__
    assert mask_module.EPS == ref.EPS
    for name in ref.__all__:
        a = inspect.signature(getattr(mask_module, name))
        b = inspect.signature(getattr(ref, name))
        assert list(a.parameters) == list(b.parameters), name
        for p in a.parameters:
            assert a.parameters[p].default == b.parameters[p].default, (name, p)
            assert a.parameters[p].kind == b.parameters[p].kind, (name, p)


def test_refusals_need_no_gpu():
    """argument checks come before the device is touched"""
    from pb_bss_amd.extraction import mask_module as mm
    x = om.gen(0, (2, 3, 4, 5))
    for fn in (mm.ideal_ratio_mask, mm.ideal_amplitude_mask, mm.phase_sensitive_mask,
               mm.ideal_complex_mask):
        with pytest.raises(AssertionError):
            fn(x, sensor_axis=1)
    with pytest.raises(AssertionError):
        mm.quantile_mask(x, sensor_axis=1)
    with pytest.raises(NotImplementedError):
        mm.biased_binary_mask(x[:, 0], sensor_axis=1)
    with pytest.raises(AssertionError):
        mm.biased_binary_mask(om.gen(0, (3, 4, 5)))


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from pb_bss_amd import _lib
    from pb_bss_amd.extraction import mask_module as mm
    x = om.gen(0, (2, 4, 20))
    for fn in (mm.ideal_binary_mask, mm.wiener_like_mask, mm.ideal_ratio_mask,
               mm.ideal_amplitude_mask, mm.phase_sensitive_mask, mm.ideal_complex_mask,
               mm.lorenz_mask, mm.quantile_mask, mm.biased_binary_mask):
        with pytest.raises(_lib.PbbssError):
            fn(x)


def test_fixtures_present():
    for name in ('pointwise', 'threshold', 'biased'):
        path = os.path.join(GOLDEN, f'mask_module_{name}.npz')
        assert os.path.getsize(path) < 1024 * 1024, path


def test_restatement_matches_recorded_pointwise():
    g = golden('pointwise')
    x = om.gen(0, (3, 4, 9, 40)).astype(np.complex128)
    xi = om.gen_integer(1, (2, 5, 11, 40)).astype(np.complex128)
    one = x[:, 0]
    assert om.ibm_ties(x, sensor_axis=1) == 0 and om.ibm_ties(x) == 0
    assert np.array_equal(om.ideal_binary_mask(x, sensor_axis=1), g['ibm_pooled'])
    assert np.array_equal(om.ideal_binary_mask(x), g['ibm'])
    assert om.ibm_ties(xi, sensor_axis=1) == 10
    assert np.array_equal(om.ideal_binary_mask(xi, sensor_axis=1), g['ibm_integer'])
    assert np.array_equal(om.wiener_like_mask(xi, sensor_axis=1), g['wiener_integer'])
    pairs = [
        (om.wiener_like_mask(x, sensor_axis=1), g['wiener_pooled']),
        (om.wiener_like_mask(x, sensor_axis=1, keepdims=True), g['wiener_pooled_keepdims']),
        (om.wiener_like_mask(x), g['wiener']),
        (om.wiener_like_mask(x, source_axis=1), g['wiener_source1']),
        (om.ideal_ratio_mask(one), g['irm']),
    ]
    for mine, ref in pairs:
        assert mine.shape == ref.shape and mine.dtype == ref.dtype
        assert np.abs(mine - ref).max() <= TOL
    amp = om.amplification(one)
    for mine, ref in [(om.ideal_amplitude_mask(one), g['iam']),
                      (om.phase_sensitive_mask(one), g['psm']),
                      (om.ideal_complex_mask(one), g['icm'])]:
        assert mine.shape == ref.shape and mine.dtype == ref.dtype
        assert (np.abs(mine - ref) <= TOL * amp).all()


def test_restatement_matches_recorded_threshold():
    g = golden('threshold')
    x = om.gen(0, (3, 4, 33, 150)).astype(np.complex128)
    xi = om.gen_integer(1, (2, 5, 11, 40)).astype(np.complex128)
    mag = np.abs(x[:, 0])
    for key, kw in [('lorenz_098', {}), ('lorenz_050', dict(lorenz_fraction=0.5)),
                    ('lorenz_last', dict(axis=-1)),
                    ('lorenz_keepdims', dict(keepdims=True, weight=0.9))]:
        d = {}
        mine = om.lorenz_mask(x, sensor_axis=1, details=d, **kw)
        om.assert_lorenz_determined(d)
        assert mine.shape == g[key].shape and np.array_equal(mine, g[key]), key
    d = {}
    mine = om.lorenz_mask(xi, sensor_axis=1, lorenz_fraction=0.9, details=d)
    om.assert_lorenz_determined(d)
    assert np.array_equal(mine, g['lorenz_integer'])
    assert (d['down'], d['up']) == (152, 728)  # equal keys at the crossing
    for key, data, q, axis in [('quantile_f', mag, (0.25, -0.5), -2),
                               ('quantile_t', mag, 0.3, -1),
                               ('quantile_ft', mag, -0.2, (-2, -1)),
                               ('quantile_default', mag, (0.1, -0.9), -2),
                               ('quantile_integer', np.abs(xi[:, 0]), (0.25, -0.5), (-2, -1))]:
        d = {}
        mine = om.quantile_mask(data, q, axis=axis, details=d)
        om.assert_quantile_determined(d)
        assert mine.shape == g[key].shape and np.array_equal(mine, g[key]), key
        if key == 'quantile_f':
            # integer virtual index: the threshold IS an element, once per row and quantile
            assert d['equal'] == 2 * 3 * 150
    assert g['quantile_default'].shape == (2, 3, 33, 150)
    with pytest.raises(ValueError):
        om.lorenz_mask(np.zeros((2, 8), np.complex128), axis=-1)


def test_restatement_matches_recorded_biased():
    g = golden('biased')
    for key, shape, kw in [
            ('biased_7_513', (2, 7, 513), {}), ('biased_513', (2, 513), {}),
            ('biased_513_args', (2, 513), dict(
                threshold_unvoiced_speech=3, threshold_voiced_speech=-2,
                threshold_unvoiced_noise=-6, threshold_voiced_noise=-12, low_cut=9,
                high_cut=400))]:
        mine = om.biased_binary_mask(biased_input(shape), **kw)
        assert mine.dtype == np.bool_ and mine.shape == g[key].shape
        assert np.array_equal(mine, g[key]), key
    # high_cut=500 reaches the array only where axis 1 of the masks is the bin axis
    assert g['biased_513'][0, 500:].sum() == 0 and g['biased_513'][1, 500:].all()
    assert g['biased_7_513'][0, :, 500:].any()


def test_voiced_unvoiced_bit_for_bit():
    from pb_bss_amd.extraction import voiced_unvoiced_split_characteristic
    g = golden('biased')
    for args in [(513,), (257,), (513, 200, 80), (129, 40, 31)]:
        key = '_'.join(str(a) for a in args)
        for fn in (voiced_unvoiced_split_characteristic, om.voiced_unvoiced_split_characteristic):
            voiced, unvoiced = fn(*args)
            assert isinstance(voiced, np.ndarray) and voiced.dtype == np.float64
            assert np.array_equal(voiced, g[f'voiced_{key}']), args
            assert np.array_equal(unvoiced, g[f'unvoiced_{key}']), args


@pytest.mark.needs_reference
def test_restatement_matches_live_reference():
    from oracle import refshim
    refshim.load()
    from pb_bss.extraction import mask_module as ref
    for seed, shape in [(11, (2, 3, 17, 21)), (12, (4, 2, 5, 64)), (13, (3, 6, 40, 9))]:
        x = om.gen(seed, shape).astype(np.complex128)
        one = x[:, 0]
        amp = om.amplification(one)
        assert np.array_equal(om.ideal_binary_mask(x, sensor_axis=1),
                              ref.ideal_binary_mask(x, sensor_axis=1))
        assert np.array_equal(om.ideal_binary_mask(x, source_axis=1, sensor_axis=0, keepdims=True),
                              ref.ideal_binary_mask(x, source_axis=1, sensor_axis=0, keepdims=True))
        assert np.abs(om.wiener_like_mask(x, sensor_axis=-3, eps=1e-3)
                      - ref.wiener_like_mask(x, sensor_axis=-3, eps=1e-3)).max() <= TOL
        assert np.abs(om.ideal_ratio_mask(one, eps=1e-6)
                      - ref.ideal_ratio_mask(one, eps=1e-6)).max() <= TOL
        assert (np.abs(om.ideal_amplitude_mask(one) - ref.ideal_amplitude_mask(one))
                <= TOL * amp).all()
        assert (np.abs(om.phase_sensitive_mask(one) - ref.phase_sensitive_mask(one))
                <= TOL * amp).all()
        assert (np.abs(om.ideal_complex_mask(one) - ref.ideal_complex_mask(one))
                <= TOL * amp).all()
        for kw in (dict(), dict(axis=(-1, 0), lorenz_fraction=0.7, weight=0.5),
                   dict(axis=(-3, -1), lorenz_fraction=0.9, keepdims=True)):
            sensor = 1 if 'keepdims' not in kw else 2
            d = {}
            mine = om.lorenz_mask(x, sensor_axis=sensor, details=d, **kw)
            om.assert_lorenz_determined(d)
            assert np.array_equal(mine, ref.lorenz_mask(x, sensor_axis=sensor, **kw)), kw
        mag = np.abs(one)
        for q, axis in [((0.1, -0.9), -2), (0.37, -1), (-0.05, (-2, -1)), ((0.0, 1.0), 0)]:
            d = {}
            mine = om.quantile_mask(mag, q, axis=axis, details=d)
            om.assert_quantile_determined(d)
            assert np.array_equal(mine, ref.quantile_mask(mag, q, axis=axis)), (q, axis)
    xb = biased_input((2, 5, 129))
    assert np.array_equal(om.biased_binary_mask(xb, high_cut=3, low_cut=2),
                          ref.biased_binary_mask(xb, high_cut=3, low_cut=2))
