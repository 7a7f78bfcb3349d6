"""GPU: pb_bss_amd.extraction.mask_module (csrc/masks.hip) against the float64 restatement of
the reference (tests/oracle_masks.py, itself pinned to the reference's recorded results by
test_mask_module_oracle.py) and against those recorded results.

The comparison target is the reference fed `signal.astype(complex128)`.  A complex128 run is
checked in float64 (bounded masks 1e-13: a D-term positive sum and one division; amplitude,
phase-sensitive and complex masks 1e-13 max(1, |s| / (|sum s| + eps)) per element); a complex64
run against that target rounded to float32, within one float32 ulp.  Binary decisions are
compared exactly, entry for entry, after the oracle has shown that the case is well determined
(Lorenz: no cumulative share within 1e-9 of the fraction; quantile: every value bit-equal to
the threshold or 1e-9 relative away from it).

One dependency on the host: the reference's Lorenz keys are np.abs(x) ** 2, and which loop
NumPy runs for np.abs of a complex array is a dispatch detail of its build.  On every x86-64
host with fused multiply-adds it is larger * sqrt(fma(q, q, 1)), q = smaller / larger, which
csrc/masks.hip reproduces bit for bit; the recorded results under tests/golden/ were written on
such a host.  Integer-valued images, whose powers tie in exact arithmetic, come apart in the
last place under that formula (152 down / 728 up at fraction 0.9; a correctly rounded hypot
gives 156 / 724).  test_lorenz_equal_keys_at_the_crossing therefore first asserts that the
live restatement still equals the recorded result: on a host whose np.abs falls back to hypot
that assertion, not the device comparison, is what fails.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle_masks as om

pytestmark = pytest.mark.gpu

TOL = 1e-13
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DTYPES = [np.complex64, np.complex128]


def torch():
    import torch as t
    return t


def mm():
    from pb_bss_amd.extraction import mask_module
    return mask_module


def host(x):
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def images(seed=0, shape=(3, 4, 33, 150)):
    x = om.gen(seed, shape)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def integer_images():
    x = om.gen_integer(1, (2, 5, 11, 40))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def long_row():
    x = om.gen(0, (1, 513, 500))
    x.setflags(write=False)
    return x


def wide(x):
    return np.asarray(x).astype(np.complex128 if np.iscomplexobj(x) else np.float64)


def close(got, ref, dtype, scale=None, what=''):
    """float64 run: |got - ref| <= TOL (* scale); float32 run: one ulp of the rounded target.
    NaN must meet NaN."""
    got = host(got)
    real = np.float32 if np.dtype(dtype) in (np.complex64, np.float32) else np.float64
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    kind = {np.float32: np.complex64, np.float64: np.complex128}[real] if np.iscomplexobj(ref) \
        else real
    assert got.dtype == kind, (what, got.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    parts = [(got.real, ref.real), (got.imag, ref.imag)] if np.iscomplexobj(ref) else [(got, ref)]
    for g, r in parts:
        if real == np.float64:
            bound = TOL * (1.0 if scale is None else scale)
            err = np.abs(g - r)
        else:
            r = r.astype(np.float32)
            bound = np.spacing(np.abs(r))
            err = np.abs(g.astype(np.float64) - r.astype(np.float64))
        worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny))[ok].max())
        print(f'{what} {np.dtype(dtype).name}: worst error / bound {worst:.3f}')
        assert (err[ok] <= np.broadcast_to(bound, err.shape)[ok]).all(), (what, worst)


# ---- pointwise ----------------------------------------------------------------------------------
def layouts():
    """name -> (images, source_axis, sensor_axis): the reference's (K, D, F, T), the
    (K, F, T, D) of stft(layout='f t d'), and a leading batch axis"""
    x = images()
    return {
        'kdft': (x, 0, 1),
        'kftd': (np.ascontiguousarray(x.transpose(0, 2, 3, 1)), 0, -1),
        'batch': (np.stack([x, images(5)]), 1, 2),
    }


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('layout', ['kdft', 'kftd', 'batch'])
def test_pooled_masks(layout, dtype):
    x, k_ax, d_ax = layouts()[layout]
    x = x.astype(dtype)
    x128 = wide(x)
    assert om.ibm_ties(x128, k_ax, d_ax) == 0
    for keepdims in (False, True):
        ibm = mm().ideal_binary_mask(x, source_axis=k_ax, sensor_axis=d_ax, keepdims=keepdims)
        ref = om.ideal_binary_mask(x128, k_ax, d_ax, keepdims)
        assert isinstance(ibm, np.ndarray) and ibm.dtype == x.real.dtype
        assert np.array_equal(ibm, ref), layout
        w = mm().wiener_like_mask(x, source_axis=k_ax, sensor_axis=d_ax, keepdims=keepdims)
        close(w, om.wiener_like_mask(x128, k_ax, d_ax, keepdims=keepdims), dtype,
              what=f'wiener {layout} keepdims={keepdims}')
    w = mm().wiener_like_mask(x, source_axis=k_ax, sensor_axis=d_ax, eps=1e-3)
    close(w, om.wiener_like_mask(x128, k_ax, d_ax, eps=1e-3), dtype, what=f'wiener eps {layout}')
    assert np.abs(host(mm().wiener_like_mask(x, k_ax, d_ax)).sum(k_ax) - 1).max() < 1e-6


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('layout', ['kdft', 'kftd', 'batch'])
def test_per_channel_masks(layout, dtype):
    """no sensor axis: every channel is an independent index"""
    x, k_ax, _ = layouts()[layout]
    x = x.astype(dtype)
    x128 = wide(x)
    amp = om.amplification(x128, k_ax)
    assert om.ibm_ties(x128, k_ax) == 0
    assert np.array_equal(mm().ideal_binary_mask(x, source_axis=k_ax),
                          om.ideal_binary_mask(x128, k_ax))
    close(mm().wiener_like_mask(x, source_axis=k_ax), om.wiener_like_mask(x128, k_ax), dtype,
          what=f'wiener {layout}')
    close(mm().ideal_ratio_mask(x, source_axis=k_ax), om.ideal_ratio_mask(x128, k_ax), dtype,
          what=f'irm {layout}')
    close(mm().ideal_ratio_mask(x, source_axis=k_ax, eps=1e-2),
          om.ideal_ratio_mask(x128, k_ax, eps=1e-2), dtype, what=f'irm eps {layout}')
    close(mm().ideal_amplitude_mask(x, source_axis=k_ax), om.ideal_amplitude_mask(x128, k_ax),
          dtype, amp, what=f'iam {layout}')
    close(mm().phase_sensitive_mask(x, source_axis=k_ax), om.phase_sensitive_mask(x128, k_ax),
          dtype, amp, what=f'psm {layout}')
    icm = mm().ideal_complex_mask(x, source_axis=k_ax)
    assert host(icm).dtype == x.dtype
    close(icm, om.ideal_complex_mask(x128, k_ax), dtype, amp, what=f'icm {layout}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('seed,shape', [(4, (3, 4, 33, 1)), (3, (1, 2, 5, 7)), (6, (2, 34, 3, 70)),
                                        (7, (9, 2, 3, 70))],
                         ids=['T1', 'K1', 'D34', 'K9'])
def test_edge_sizes(seed, shape, dtype):
    x = images(seed, shape).astype(dtype)
    x128 = wide(x)
    assert om.ibm_ties(x128, 0, 1) == 0
    assert np.array_equal(mm().ideal_binary_mask(x, sensor_axis=1),
                          om.ideal_binary_mask(x128, 0, 1))
    close(mm().wiener_like_mask(x, sensor_axis=1), om.wiener_like_mask(x128, 0, 1), dtype,
          what=f'wiener {shape}')
    xt = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    close(mm().wiener_like_mask(xt, sensor_axis=-1), om.wiener_like_mask(wide(xt), 0, -1), dtype,
          what=f'wiener {shape} sensors last')
    one, one128 = x[:, 0], x128[:, 0]
    amp = om.amplification(one128)
    close(mm().ideal_ratio_mask(one), om.ideal_ratio_mask(one128), dtype, what=f'irm {shape}')
    close(mm().ideal_amplitude_mask(one), om.ideal_amplitude_mask(one128), dtype, amp,
          what=f'iam {shape}')
    close(mm().phase_sensitive_mask(one), om.phase_sensitive_mask(one128), dtype, amp,
          what=f'psm {shape}')
    close(mm().ideal_complex_mask(one), om.ideal_complex_mask(one128), dtype, amp,
          what=f'icm {shape}')


def test_size_limits():
    with pytest.raises(NotImplementedError):
        mm().wiener_like_mask(images(8, (10, 2, 3, 5)))
    with pytest.raises(NotImplementedError):
        mm().wiener_like_mask(images(8, (2, 35, 3, 5)), sensor_axis=1)
    with pytest.raises(NotImplementedError):
        mm().lorenz_mask(images(8, (2, 35, 3, 5)), sensor_axis=1)


@pytest.mark.parametrize('dtype', DTYPES)
def test_recorded_reference_pointwise(dtype):
    g = np.load(os.path.join(GOLDEN, 'mask_module_pointwise.npz'))
    x = om.gen(0, (3, 4, 9, 40)).astype(dtype)
    one = x[:, 0]
    amp = om.amplification(wide(one))
    assert np.array_equal(mm().ideal_binary_mask(x, sensor_axis=1), g['ibm_pooled'])
    assert np.array_equal(mm().ideal_binary_mask(x), g['ibm'])
    close(mm().wiener_like_mask(x, sensor_axis=1), g['wiener_pooled'], dtype, what='wiener')
    close(mm().wiener_like_mask(x, sensor_axis=1, keepdims=True), g['wiener_pooled_keepdims'],
          dtype, what='wiener keepdims')
    close(mm().wiener_like_mask(x, source_axis=1), g['wiener_source1'], dtype, what='wiener k=1')
    close(mm().ideal_ratio_mask(one), g['irm'], dtype, what='irm')
    close(mm().ideal_amplitude_mask(one), g['iam'], dtype, amp, what='iam')
    close(mm().phase_sensitive_mask(one), g['psm'], dtype, amp, what='psm')
    close(mm().ideal_complex_mask(one), g['icm'], dtype, amp, what='icm')


@pytest.mark.parametrize('dtype', DTYPES)
def test_ties_go_to_the_first_source(dtype):
    g = np.load(os.path.join(GOLDEN, 'mask_module_pointwise.npz'))
    x = integer_images().astype(dtype)
    assert om.ibm_ties(wide(x), 0, 1) == 10  # points at which both sources have the same power
    ibm = mm().ideal_binary_mask(x, sensor_axis=1)
    assert np.array_equal(ibm, g['ibm_integer'])
    p = (wide(x).real ** 2 + wide(x).imag ** 2).sum(1)
    tied = p[0] == p[1]
    assert tied.sum() == 10 and (ibm[0][tied] == 1).all() and (ibm[1][tied] == 0).all()
    # integer powers: the Wiener-like mask is one exactly rounded quotient
    w = mm().wiener_like_mask(x, sensor_axis=1)
    ref = g['wiener_integer']
    assert np.array_equal(w, ref.astype(w.dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_silent_points(dtype):
    x = images().astype(dtype).copy()
    quiet = [(0, 0), (5, 7), (32, 149), (17, 64)]
    for f, t in quiet:
        x[:, :, f, t] = 0
    one = x[:, 0]
    ibm = mm().ideal_binary_mask(x, sensor_axis=1)
    w = mm().wiener_like_mask(x, sensor_axis=1)
    irm = mm().ideal_ratio_mask(one)
    iam = mm().ideal_amplitude_mask(one)
    psm = mm().phase_sensitive_mask(one)
    close(psm, om.phase_sensitive_mask(wide(one)), dtype, om.amplification(wide(one)), what='psm')
    icm = mm().ideal_complex_mask(one)
    for f, t in quiet:
        assert list(ibm[:, f, t]) == [1, 0, 0]
        assert (w[:, f, t] == 0).all() and (irm[:, f, t] == 0).all() and (iam[:, f, t] == 0).all()
        assert (psm[:, f, t] == 0).all()
        assert np.isnan(icm[:, f, t].real).all() and np.isnan(icm[:, f, t].imag).all()
    assert np.isnan(icm.real).sum() == 3 * len(quiet)
    close(icm, om.ideal_complex_mask(wide(one)), dtype, om.amplification(wide(one)), what='icm')


def biased_input(shape):
    x = om.gen(2, shape).astype(np.complex128)
    x[1] *= 0.3
    return x


@pytest.mark.parametrize('dtype', DTYPES)
def test_biased_binary_mask(dtype):
    g = np.load(os.path.join(GOLDEN, 'mask_module_biased.npz'))
    args = dict(threshold_unvoiced_speech=3, threshold_voiced_speech=-2,
                threshold_unvoiced_noise=-6, threshold_voiced_noise=-12, low_cut=9, high_cut=400)
    for key, shape, kw in [('biased_7_513', (2, 7, 513), {}), ('biased_513', (2, 513), {}),
                           ('biased_513_args', (2, 513), args)]:
        x = biased_input(shape)
        if dtype == np.complex64:
            # the recorded result belongs to the complex128 images: take the float32 images
            # only if rounding them moves no decision
            x = x.astype(np.complex64)
            d = {}
            ref = om.biased_binary_mask(wide(x), details=d, **kw)
            assert d['gap'] > 1e-12 and np.array_equal(ref, g[key])
        m = mm().biased_binary_mask(x, **kw)
        assert isinstance(m, np.ndarray) and m.dtype == np.bool_ and m.shape == g[key].shape
        assert np.array_equal(m, g[key]), key
    # another component axis, and a device tensor
    x = biased_input((2, 7, 513))
    xd = torch().from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).cuda()
    m = mm().biased_binary_mask(xd, component_axis=1)
    assert m.is_cuda and m.dtype == torch().bool
    assert np.array_equal(host(m), om.biased_binary_mask(x.transpose(1, 0, 2), component_axis=1))


# ---- Lorenz ---------------------------------------------------------------------------------------
def lorenz_oracle(x, **kw):
    d = {}
    ref = om.lorenz_mask(wide(x), details=d, **kw)
    om.assert_lorenz_determined(d)  # precondition of an exact comparison
    return ref, d


def equal_masks(got, ref, dtype, what):
    got = host(got)
    real = np.float32 if np.dtype(dtype) in (np.complex64, np.float32) else np.float64
    assert got.dtype == real and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    wrong = int((got != ref.astype(real)).sum())
    print(f'{what} {np.dtype(dtype).name}: {wrong} of {ref.size} entries differ')
    assert wrong == 0, what


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('fraction', [0.98, 0.5])
def test_lorenz_pooled(fraction, dtype):
    """3 rows of 4950 values: the multi-pass selection, in both layouts"""
    x = images().astype(dtype)
    ref, d = lorenz_oracle(x, sensor_axis=1, lorenz_fraction=fraction)
    print(f'fraction {fraction}: margin {d["margin"]:.2e}, {d["down"]} down, {d["up"]} up')
    equal_masks(mm().lorenz_mask(x, sensor_axis=1, lorenz_fraction=fraction), ref, dtype, 'kdft')
    xt = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    equal_masks(mm().lorenz_mask(xt, sensor_axis=-1, axis=(1, 2), lorenz_fraction=fraction), ref,
                dtype, 'kftd')
    if fraction == 0.98:
        g = np.load(os.path.join(GOLDEN, 'mask_module_threshold.npz'))
        assert np.array_equal(ref, g['lorenz_098'])


@pytest.mark.parametrize('dtype', DTYPES)
def test_lorenz_long_row(dtype):
    """one row of 513 * 500 values, seed 0 (margin 3.6e-7)"""
    x = long_row().astype(dtype)
    ref, d = lorenz_oracle(x)
    print(f'margin {d["margin"]:.2e}, {d["down"]} down, {d["up"]} up')
    equal_masks(mm().lorenz_mask(x), ref, dtype, 'long row')


@pytest.mark.parametrize('dtype', DTYPES)
def test_lorenz_equal_keys_at_the_crossing(dtype):
    g = np.load(os.path.join(GOLDEN, 'mask_module_threshold.npz'))
    x = integer_images().astype(dtype)
    ref, d = lorenz_oracle(x, sensor_axis=1, lorenz_fraction=0.9)
    assert (d['down'], d['up']) == (152, 728) and np.array_equal(ref, g['lorenz_integer'])
    equal_masks(mm().lorenz_mask(x, sensor_axis=1, lorenz_fraction=0.9), ref, dtype, 'integer')
    # the same rows, long enough for the multi-pass path: every row five times over
    big = np.tile(x, (1, 1, 5, 1))
    ref, d = lorenz_oracle(big, sensor_axis=1, lorenz_fraction=0.9)
    equal_masks(mm().lorenz_mask(big, sensor_axis=1, lorenz_fraction=0.9), ref, dtype, 'tiled')


@pytest.mark.parametrize('dtype', DTYPES)
def test_lorenz_axes_and_keepdims(dtype):
    g = np.load(os.path.join(GOLDEN, 'mask_module_threshold.npz'))
    x = images().astype(dtype)
    ref, _ = lorenz_oracle(x, sensor_axis=1, axis=-1)
    assert np.array_equal(ref, g['lorenz_last'])
    equal_masks(mm().lorenz_mask(x, sensor_axis=1, axis=-1), ref, dtype, 'axis=-1')
    ref, _ = lorenz_oracle(x, sensor_axis=1, axis=-2)
    equal_masks(mm().lorenz_mask(x, sensor_axis=1, axis=-2), ref, dtype, 'axis=-2')
    ref, _ = lorenz_oracle(x, sensor_axis=1, keepdims=True, weight=0.9)
    assert np.array_equal(ref, g['lorenz_keepdims']) and ref.shape == (3, 1, 33, 150)
    equal_masks(mm().lorenz_mask(x, sensor_axis=1, keepdims=True, weight=0.9), ref, dtype,
                'keepdims')
    # no pooling: every channel its own row
    ref, _ = lorenz_oracle(x)
    equal_masks(mm().lorenz_mask(x), ref, dtype, 'per channel')


def test_lorenz_without_a_threshold_raises():
    x = images().copy()
    x[1] = 0
    with pytest.raises(ValueError):
        mm().lorenz_mask(x, sensor_axis=1)
    with pytest.raises(ValueError):
        mm().lorenz_mask(x, sensor_axis=1, axis=-1)  # rows of 150: the one-launch path
    long = long_row().copy()
    long[:] = 0
    long[0, 3, 4] = 1  # one element carries everything
    with pytest.raises(ValueError):
        mm().lorenz_mask(long)


# ---- quantile -------------------------------------------------------------------------------------
def quantile_oracle(v, q, axis):
    d = {}
    ref = om.quantile_mask(wide(v), q, axis=axis, details=d)
    om.assert_quantile_determined(d)
    return ref, d


@pytest.mark.parametrize('dtype', [np.float32, np.float64, np.complex64])
@pytest.mark.parametrize('axis', [-2, -1, (-2, -1)], ids=['f', 't', 'ft'])
def test_quantile_axes(axis, dtype):
    x = images()[:, 0]
    v = x if dtype == np.complex64 else np.abs(x).astype(dtype)
    for q in [(0.25, -0.5), (0.1, -0.9), 0.3, -0.2, 0.0, 1.0, -1.0]:
        # the complex images go through the device's own |x| (float64 of the widened values,
        # the path a user of the module takes); the oracle takes np.abs of the same values
        ref, d = quantile_oracle(np.abs(wide(v)), q, axis)
        got = mm().quantile_mask(v, q, axis=axis)
        equal_masks(got, ref, dtype, f'q={q} axis={axis} ({d["equal"]} equal to the threshold)')
        if axis == -2 and q == (0.25, -0.5) and dtype != np.complex64:
            assert d['equal'] == 2 * 3 * 150  # integer virtual index: the strict comparison
    ref, _ = quantile_oracle(np.abs(wide(v)), (0.1, -0.9), -2)
    got = mm().quantile_mask(v)
    assert got.shape == (2, 3, 33, 150)
    equal_masks(got, ref, dtype, 'defaults')
    ref = om.quantile_mask(np.abs(wide(v)), (0.1, -0.9), axis=axis, weight=0.5)
    equal_masks(mm().quantile_mask(v, axis=axis, weight=0.5), ref, dtype, 'weight')


def test_quantile_row_with_a_nan():
    """np.percentile of a row that holds a NaN is NaN, and nothing is above or below NaN: the
    whole row is rated down, for either sign (one-launch path, rows of 33); the rows without a
    NaN are untouched"""
    v = np.abs(wide(images()[:, 0]))            # (3, 33, 150)
    v[1, 5, 7] = np.nan
    with np.errstate(invalid='ignore'):
        ref = om.quantile_mask(v, (0.25, -0.5), axis=-2)
    assert (ref[:, 1, :, 7] == ref.min()).all()
    got = mm().quantile_mask(v, (0.25, -0.5), axis=-2)
    equal_masks(got, ref, np.float64, 'row of 33 with a NaN')


def test_quantile_recorded_reference():
    g = np.load(os.path.join(GOLDEN, 'mask_module_threshold.npz'))
    mag = np.abs(wide(images()[:, 0]))
    assert np.array_equal(mm().quantile_mask(mag, (0.25, -0.5), axis=-2), g['quantile_f'])
    assert np.array_equal(mm().quantile_mask(mag, 0.3, axis=-1), g['quantile_t'])
    assert np.array_equal(mm().quantile_mask(mag, -0.2, axis=(-2, -1)), g['quantile_ft'])
    assert np.array_equal(mm().quantile_mask(mag), g['quantile_default'])
    xi = np.abs(wide(integer_images()[:, 0]))
    assert np.array_equal(mm().quantile_mask(xi, (0.25, -0.5), axis=(-2, -1)),
                          g['quantile_integer'])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_quantile_long_row_and_whole_array(dtype):
    v = np.abs(long_row()).astype(dtype)
    ref, d = quantile_oracle(v, (0.1, -0.9), (-2, -1))
    equal_masks(mm().quantile_mask(v, axis=(-2, -1)), ref, dtype, f'long row, gap {d["gap"]:.1e}')
    # every axis consumed: one row (the reference fails here under NumPy 2)
    got = mm().quantile_mask(v, axis=(0, 1, 2))
    equal_masks(got, ref, dtype, 'all axes')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_quantile_integer_ties(dtype):
    xi = np.abs(integer_images()).astype(dtype)
    for axis in [(-2, -1), -1, (-3, -2, -1)]:
        ref, d = quantile_oracle(xi, (0.25, -0.5), axis)
        assert d['equal'] > 0
        equal_masks(mm().quantile_mask(xi, (0.25, -0.5), axis=axis), ref, dtype,
                    f'integer axis={axis} ({d["equal"]} equal)')
    many = tuple(np.linspace(-0.95, 0.95, 11).round(3))  # more than one sweep of eight
    ref, _ = quantile_oracle(xi, many, (-3, -2, -1))
    equal_masks(mm().quantile_mask(xi, many, axis=(-3, -2, -1)), ref, dtype, 'eleven quantiles')
    with pytest.raises(ValueError):
        mm().quantile_mask(xi, 1.5)


# ---- plumbing ---------------------------------------------------------------------------------------
def test_device_in_device_out_and_strided_views():
    t = torch()
    x = images()
    xd = t.from_numpy(x.copy()).cuda()
    ref = om.wiener_like_mask(wide(x), 0, 1)
    w = mm().wiener_like_mask(xd, sensor_axis=1)
    assert w.is_cuda and w.device == xd.device and w.dtype == t.float32
    close(w, ref, np.complex64, what='device')
    assert isinstance(mm().wiener_like_mask(x, sensor_axis=1), np.ndarray)
    # a transposed view is read where it lies (no copy: the strides go to the kernel)
    view = xd.permute(0, 2, 3, 1)
    assert not view.is_contiguous()
    close(mm().wiener_like_mask(view, sensor_axis=-1), ref, np.complex64, what='view')
    close(mm().wiener_like_mask(xd.permute(2, 0, 3, 1), source_axis=1, sensor_axis=3),
          np.moveaxis(ref, 1, 0), np.complex64, what='view, sources second')
    # five strided groups: one copy, same result
    big = t.from_numpy(om.gen(9, (2, 3, 2, 4, 3, 5, 6))).cuda()
    odd = big[:, :, :, :, :, :, ::2].permute(4, 1, 0, 3, 2, 6, 5)
    got = mm().wiener_like_mask(odd, source_axis=1, sensor_axis=3)
    close(got, om.wiener_like_mask(wide(host(odd)), 1, 3), np.complex64, what='copy path')
    lm = mm().lorenz_mask(view, sensor_axis=-1, axis=(1, 2))
    assert lm.is_cuda and lm.dtype == t.float32
    equal_masks(lm, lorenz_oracle(x, sensor_axis=1)[0], np.complex64, 'lorenz view')
    qm = mm().quantile_mask(xd[:, 0].to(t.complex128), axis=-2)
    assert qm.is_cuda and qm.dtype == t.float64 and tuple(qm.shape) == (2, 3, 33, 150)
    equal_masks(qm, quantile_oracle(np.abs(wide(x[:, 0])), (0.1, -0.9), -2)[0], np.complex128,
                'quantile device')
    strided = t.from_numpy(np.abs(x)).cuda().permute(1, 3, 0, 2)  # (D, T, K, F)
    equal_masks(mm().quantile_mask(strided, 0.2, axis=1),
                quantile_oracle(np.abs(wide(x)).transpose(1, 3, 0, 2), 0.2, 1)[0], np.float32,
                'quantile strided')
    assert mm().ideal_binary_mask(xd.to(t.complex128), sensor_axis=1).dtype == t.float64
    assert mm().ideal_complex_mask(xd[:, 0]).dtype == t.complex64


def test_mask_feeds_the_psd_kernel():
    """device images -> Wiener-like mask -> get_power_spectral_density_matrix, no host hop"""
    from oracle import beamformer as ob
    from pb_bss_amd import extraction as ex
    t = torch()
    x = wide(images())                       # (K, D, F, T)
    xd = t.from_numpy(x).cuda()
    mask = ex.wiener_like_mask(xd, sensor_axis=1)      # (K, F, T), stays on the device
    assert mask.is_cuda
    obs = xd.sum(0).permute(1, 0, 2)                    # (F, D, T)
    psd = ex.get_power_spectral_density_matrix(obs, mask.permute(1, 0, 2))
    assert psd.is_cuda and tuple(psd.shape) == (33, 3, 4, 4)
    ref_mask = om.wiener_like_mask(x, 0, 1)
    ref = ob.psd(x.sum(0).transpose(1, 0, 2), ref_mask.transpose(1, 0, 2))
    err = float(np.abs(host(psd) - ref).max())
    print(f'PSD from the device mask vs from the reference mask: {err:.2e}')
    assert err <= 1e-10


def test_c_abi_refuses_bad_shapes():
    t = torch()
    from pb_bss_amd import _lib
    lib, h, stream = _lib.load(), _lib.handle(0), _lib.stream_ptr(0)
    x = t.zeros((2, 4, 64), dtype=t.complex64, device='cuda')
    out = t.zeros((2, 64), dtype=t.float32, device='cuda')
    st = t.zeros((2,), dtype=t.int32, device='cuda')

    def geom(K=2, D=4, n=64):
        g = _lib.MaskGeom()
        for i, (size, xs, os_) in enumerate([(1, 0, 0), (1, 0, 0), (1, 0, 0), (n, 1, 1)]):
            g.size[i], g.x_stride[i], g.out_stride[i] = size, xs, os_
        g.sources, g.sensors = K, D
        g.x_source_stride, g.x_sensor_stride, g.out_source_stride = 256, 64, 64
        return g

    def pointwise(g, mode=_lib.MASK_WIENER, xx=x, oo=out, handle=h, table=None):
        return lib.pbbss_mask_pointwise(handle, _lib.ptr(xx), 0, mode, ctypes.byref(g) if g else
                                        None, 1e-18, table, 0, _lib.ptr(oo), stream)
    assert pointwise(geom()) == _lib.OK
    assert pointwise(geom(K=10)) == _lib.ERR_UNSUPPORTED
    assert pointwise(geom(D=35)) == _lib.ERR_UNSUPPORTED
    assert pointwise(geom(), mode=_lib.MASK_BIASED, table=_lib.ptr(st)) == _lib.ERR_INVALID_ARG
    assert pointwise(geom(K=0)) == _lib.ERR_INVALID_ARG
    assert pointwise(geom(n=0)) == _lib.ERR_INVALID_ARG
    assert pointwise(geom(), mode=7) == _lib.ERR_INVALID_ARG
    assert pointwise(None) == _lib.ERR_INVALID_ARG
    assert pointwise(geom(), xx=None) == _lib.ERR_INVALID_ARG
    assert pointwise(geom(), handle=None) == _lib.ERR_INVALID_ARG
    assert b'shape' in lib.pbbss_error_string(pointwise(geom(K=10)))

    def lorenz(g, status=st):
        return lib.pbbss_mask_lorenz(h, _lib.ptr(x), 0, ctypes.byref(g), 0.98, 0.9995, 0.0005,
                                     _lib.ptr(out), 0, _lib.ptr(status), stream)
    g = geom()
    g.size[1], g.x_stride[1], g.out_stride[1] = 2, 256, 64
    assert lorenz(g) == _lib.OK
    g.sensors = 35
    assert lorenz(g) == _lib.ERR_UNSUPPORTED
    g.sensors = 4
    assert lorenz(g, status=None) == _lib.ERR_INVALID_ARG

    def quantile(g, n=1, rank=0, gamma=0.0):
        ranks = (ctypes.c_int64 * 9)(*([rank] * 9))
        gammas = (ctypes.c_double * 9)(*([gamma] * 9))
        neg = (ctypes.c_int * 9)()
        return lib.pbbss_mask_quantile(h, _lib.ptr(x), 0, ctypes.byref(g), n, ranks, gammas, neg,
                                       0.9995, 0.0005, _lib.ptr(out), 0, _lib.ptr(st), stream)
    g.sensors = 1
    g.out_target_stride = 0
    assert quantile(g) == _lib.OK
    assert quantile(g, n=9) == _lib.ERR_UNSUPPORTED
    assert quantile(g, n=0) == _lib.ERR_INVALID_ARG
    assert quantile(g, rank=64) == _lib.ERR_INVALID_ARG
    assert quantile(g, gamma=1.0) == _lib.ERR_INVALID_ARG
    g.sensors = 4
    assert quantile(g) == _lib.ERR_UNSUPPORTED
    t.cuda.synchronize()
