"""GPU: the complex circular-symmetric Gaussian (csrc/ccsg.hip) against the reference fixtures,
the float64 oracle of tests/oracle_ccsg.py and its longdouble restatement.  Everything goes
through the C ABI; the premises (oracle = reference, what the sweep reaches, the table below) are
checked on the CPU by tests/test_ccsg_oracle.py.

Tolerances.
  covariance  |delta| <= (N + 4) 2^-52 max_d C_dd per matrix, against the longdouble restatement
              (any summation order of N products has error <= N u sum|terms|, and
              sum_n s |y_d y_e| / den <= sqrt(C_dd C_ee)); exactly Hermitian, exactly real diagonal.
  log-pdf     rtol 1e-9 / atol 1e-7 on well-conditioned covariances (the package's log-pdf
              tolerance, tests/test_gpu_gauss_full.py), log-determinant rtol 1e-10 there.  On the
              conditioning cases the larger of that and 32 x the oracle's own error x max|log_pdf|:
              two backward-stable factorisations of one float64 matrix that differ in elimination
              and summation order.  The oracle's error against longdouble, relative to
              max|log_pdf|, worst of D = 3, 8, 16, 34 (measured by tests/test_ccsg_oracle.py):
                  cond 1e2: 1.6e-15    cond 1e6: 7.3e-13    cond 1e10: 9.7e-09
"""
import ctypes

import numpy as np
import pytest

import oracle_ccsg as oc

pytestmark = pytest.mark.gpu

LOG_PDF_ORACLE_ERROR = {1e2: 1.6e-15, 1e6: 7.3e-13, 1e10: 9.7e-09}


@pytest.fixture(scope='module')
def dev():
    from pb_bss_amd import _lib, engine
    _lib.require_gpu()
    return _lib, engine


def check_covariance(got, y, s, what):
    """(B, K, D, D) against the longdouble restatement of the fit of y (B, N, D), s (B, K, N)."""
    want = oc.oracle_fit(y, s, oc.fit_ext)
    N = y.shape[-2]
    diag = np.einsum('...dd->...d', want).real.max(axis=-1).astype(np.float64)
    tol = (N + 4) * 2.0 ** -52 * diag[..., None, None]
    err = np.abs(got - want).astype(np.float64)
    print(f'{what}: cov err {(err / np.maximum(tol, 1e-300)).max():.2f} of the bound')
    assert got.dtype == np.complex128 and got.shape == want.shape, what
    assert (err <= tol).all(), what
    assert (got == np.swapaxes(got.conj(), -1, -2)).all(), what
    assert (np.einsum('...dd->...d', got).imag == 0).all(), what


def check_log_pdf(lp, ref, what, oracle_error=0.0):
    extra = 32 * oracle_error * np.abs(ref).max()
    print(f'{what}: log-pdf err {np.abs(lp - ref).max():.2e}, max|log_pdf| {np.abs(ref).max():.2e}, '
          f'extra tolerance {extra:.1e}')
    assert lp.shape == ref.shape, what
    assert (np.abs(lp - ref) <= np.maximum(1e-7 + 1e-9 * np.abs(ref), extra)).all(), what


def run_fit(dev, y, s):
    _lib, engine = dev
    return _lib.to_host(engine.ccsg_fit(_lib.to_device(y), None if s is None else _lib.to_device(s)))


def run_log_pdf(dev, y, cov):
    _lib, engine = dev
    lp, ld, st = engine.ccsg_log_pdf(_lib.to_device(y), _lib.to_device(cov), want_log_det=True)
    return _lib.to_host(lp), _lib.to_host(ld), _lib.to_host(st)


@pytest.mark.parametrize('D', oc.D_SWEEP)
def test_shape_sweep(dev, D):
    fixture_keys = {oc.case_key(*c) for c in oc.FIXTURE_CASES}
    for N, K, B, y_dtype, sal_dtype in oc.sweep_cases(D):
        y, s, cov = oc.case(D, N, K, B, y_dtype, sal_dtype)
        key = oc.case_key(D, N, K, B, y_dtype, sal_dtype)
        got = run_fit(dev, y, s)
        check_covariance(got, y, s, key)
        lp, ld, st = run_log_pdf(dev, y, cov)
        assert (st == 0).all(), key
        if key in fixture_keys:
            fx = oc.fixtures()
            # the reference's own float64 sum carries the bound of check_covariance as well
            diag = np.einsum('...dd->...d', fx[key + '/cov']).real.max(axis=-1)
            tol = 2 * (N + 4) * 2.0 ** -52 * diag[..., None, None]
            assert (np.abs(got - fx[key + '/cov']) <= tol).all(), key
            check_log_pdf(lp, fx[key + '/lp'], key + ' (fixture)')
        ref = oc.log_pdf(y[:, None], cov)
        check_log_pdf(lp, ref, key)
        np.testing.assert_allclose(ld, np.linalg.slogdet(cov)[1], rtol=1e-10, atol=1e-12,
                                   err_msg=key)


@pytest.mark.parametrize('cond', oc.CONDITIONS)
def test_conditioning(dev, cond):
    for D in oc.CONDITION_DS:
        y, c = oc.conditioned(cond, D)
        for dtype in oc.Y_DTYPES:
            yd = y.astype(dtype)
            lp, ld, st = run_log_pdf(dev, yd[None], c[None, None])
            assert (st == 0).all()
            check_log_pdf(lp[0, 0], oc.log_pdf(yd, c), f'cond {cond:g} D {D} {np.dtype(dtype).name}',
                          oracle_error=LOG_PDF_ORACLE_ERROR[cond])
            # the quadratic form is a sum of squares: never negative
            assert (lp[0, 0] <= -D * np.log(np.pi) - ld[0, 0] + 1e-12).all()


def test_bit_for_bit(dev):
    _lib, engine = dev
    for D, N, K, B in ((3, 65, 3, 2), (8, 300, 9, 2), (16, 129, 3, 1), (34, 257, 7, 1)):
        y, s, cov = oc.case(D, N, K, B, np.complex64, np.float32)
        yd, sd, cd = _lib.to_device(y), _lib.to_device(s), _lib.to_device(cov)
        # two identical calls (N beyond one span: the partial sums of the fit are combined)
        assert N > engine.ccsg_frames(D) or D == 3
        a, b = engine.ccsg_fit(yd, sd), engine.ccsg_fit(yd, sd)
        assert bool((a.view(_lib.torch().float64) == b.view(_lib.torch().float64)).all())
        lp, ld, _ = engine.ccsg_log_pdf(yd, cd, want_log_det=True)
        lp2, ld2, _ = engine.ccsg_log_pdf(yd, cd, want_log_det=True)
        assert bool((lp == lp2).all()) and bool((ld == ld2).all())
        # complex64 values passed as complex128
        wide = _lib.to_device(y.astype(np.complex128))
        assert bool((engine.ccsg_log_pdf(wide, cd)[0] == lp).all())
        c = engine.ccsg_fit(wide, _lib.to_device(s.astype(np.float64)))
        assert bool((c.view(_lib.torch().float64) == a.view(_lib.torch().float64)).all())
        # class k of the (B, K) call is the (B, 1) call on that class's covariance
        for k in range(K):
            alone, ld1, _ = engine.ccsg_log_pdf(yd, cd[:, k:k + 1].contiguous(), want_log_det=True)
            assert bool((alone[:, 0] == lp[:, k]).all()) and bool((ld1[:, 0] == ld[:, k]).all())


def test_broadcasting_and_tensor_kinds(dev):
    _lib, _ = dev
    from pb_bss_amd.distribution import (ComplexCircularSymmetricGaussian,
                                         ComplexCircularSymmetricGaussianTrainer)
    trainer = ComplexCircularSymmetricGaussianTrainer()
    F, K, N, D = 4, 3, 70, 5
    y = oc.frames(1, (F, N, D))
    s = oc.saliency(1, (F, K, N))
    cov = oc.spd(1, (F, K), D)
    # mixture layout
    m = trainer.fit(y[:, None], saliency=s)
    assert isinstance(m, ComplexCircularSymmetricGaussian) and m.covariance.shape == (F, K, D, D)
    assert isinstance(m.covariance, np.ndarray) and m.covariance.dtype == np.complex128
    check_covariance(m.covariance, y, s, 'fit (F,1,N,D) x (F,K,N)')
    lp = ComplexCircularSymmetricGaussian(covariance=cov).log_pdf(y[:, None])
    assert isinstance(lp, np.ndarray) and lp.dtype == np.float64
    check_log_pdf(lp, oc.log_pdf(y[:, None], cov), 'log_pdf (F,1,N,D) x (F,K,D,D)')
    # one matrix
    m = trainer.fit(y[0])
    assert m.covariance.shape == (D, D)
    check_covariance(m.covariance[None, None], y[:1], None, 'fit (N,D)')
    m = trainer.fit(y[0], saliency=s[0, 0])
    check_covariance(m.covariance[None, None], y[:1], s[:1, :1], 'fit (N,D) x (N,)')
    lp = ComplexCircularSymmetricGaussian(covariance=cov[0, 0]).log_pdf(y[0])
    check_log_pdf(lp, oc.log_pdf(y[0], cov[0, 0]), 'log_pdf (N,D) x (D,D)')
    # one matrix against a batch of observations; one saliency against the batch
    lp = ComplexCircularSymmetricGaussian(covariance=cov[0, 0]).log_pdf(y)
    check_log_pdf(lp, oc.log_pdf(y, cov[0, 0]), 'log_pdf (F,N,D) x (D,D)')
    m = trainer.fit(y, saliency=s[0, 0])
    assert m.covariance.shape == (F, D, D)
    check_covariance(m.covariance[:, None], y, np.broadcast_to(s[0, 0], (F, 1, N)),
                     'fit (F,N,D) x (N,)')
    m = trainer.fit(y)
    check_covariance(m.covariance[:, None], y, None, 'fit (F,N,D)')
    # classes against one observation matrix
    lp = ComplexCircularSymmetricGaussian(covariance=cov[0]).log_pdf(y[0])
    check_log_pdf(lp, oc.log_pdf(y[0], cov[0]), 'log_pdf (N,D) x (K,D,D)')
    # device tensors in, device tensors out
    t = _lib.torch()
    yt, st = _lib.to_device(y[:, None]), _lib.to_device(s)
    mt = trainer.fit(yt, saliency=st)
    assert t.is_tensor(mt.covariance) and mt.covariance.is_cuda
    lpt = mt.log_pdf(yt)
    assert t.is_tensor(lpt) and lpt.is_cuda and lpt.shape == (F, K, N)
    check_log_pdf(_lib.to_host(lpt), oc.log_pdf(y[:, None], oc.fit(y[:, None], s)), 'tensors')


def test_reference_result_dtypes(dev):
    from pb_bss_amd.distribution import ComplexCircularSymmetricGaussianTrainer
    from pb_bss_amd.distribution.utils import result_dtype
    trainer = ComplexCircularSymmetricGaussianTrainer()
    y = oc.frames(2, (3, 1, 40, 4), np.complex64)
    s32 = oc.saliency(2, (3, 2, 40), np.float32)
    assert trainer.fit(y, saliency=s32).covariance.dtype == np.complex128
    with result_dtype('reference'):
        assert trainer.fit(y).covariance.dtype == np.complex64
        m = trainer.fit(y, saliency=s32)
        assert m.covariance.dtype == np.complex64
        assert trainer.fit(y, saliency=s32.astype(np.float64)).covariance.dtype == np.complex128
        assert trainer.fit(y.astype(np.complex128), saliency=s32).covariance.dtype == np.complex128
        assert m.log_pdf(y).dtype == np.float32
    np.testing.assert_allclose(m.covariance, oc.fit(y, s32), rtol=1e-6, atol=1e-7)


def test_status(dev):
    from pb_bss_amd.distribution import (ComplexCircularSymmetricGaussian,
                                         ComplexCircularSymmetricGaussianTrainer)
    _lib, engine = dev
    D, N = 3, 50
    y = oc.frames(3, (2, 1, N, D))
    good = oc.spd(3, (2, 4), D)
    for bad in (np.zeros((D, D)), np.diag([1.0, -2.0, 3.0])):
        cov = good.copy()
        cov[1, 2] = bad
        with pytest.raises(np.linalg.LinAlgError):
            ComplexCircularSymmetricGaussian(covariance=cov).log_pdf(y)
        lp, ld, st = run_log_pdf(dev, y[:, 0], cov)
        assert st[1, 2] == _lib.ST_NOT_POSDEF and np.count_nonzero(st) == 1
        assert np.isnan(lp[1, 2]).all() and np.isnan(ld[1, 2])
        ref = oc.log_pdf(y, good)
        ref[1, 2] = lp[1, 2]
        np.testing.assert_allclose(lp, ref, rtol=1e-9, atol=1e-7)
    # a NaN in one covariance: that row only, no exception
    cov = good.copy()
    cov[0, 1, 2, 0] = np.nan
    lp = ComplexCircularSymmetricGaussian(covariance=cov).log_pdf(y)
    assert np.isnan(lp[0, 1]).all()
    lp[0, 1] = 0
    assert np.isfinite(lp).all()
    _, _, st = run_log_pdf(dev, y[:, 0], cov)
    assert st[0, 1] == _lib.ST_NONFINITE and np.count_nonzero(st) == 1
    # only the lower triangle and the real diagonal are read
    cov = good.copy()
    cov[..., 0, 2] = np.nan
    cov[..., 1, 1] += 5j
    assert (run_log_pdf(dev, y[:, 0], cov)[0] == run_log_pdf(dev, y[:, 0], good)[0]).all()
    # a NaN frame of zero saliency reaches the covariance row / column of its sensor
    s = oc.saliency(3, (2, 3, N))
    s[:, 1, 7] = 0
    yn = y.copy()
    yn[0, 0, 7, 2] = np.nan
    c = ComplexCircularSymmetricGaussianTrainer().fit(yn, saliency=s).covariance
    assert np.isnan(c[0, :, 2, :]).all() and np.isnan(c[0, :, :, 2]).all()
    assert np.isfinite(c[0, :, :2, :2]).all() and np.isfinite(c[1]).all()
    # a zero saliency sum: exactly zero
    s[1, 2] = 0
    c = ComplexCircularSymmetricGaussianTrainer().fit(y, saliency=s).covariance
    assert (c[1, 2] == 0).all() and np.abs(c[1, 1]).max() > 0


def test_host_plumbing(dev):
    from pb_bss_amd import distribution as dist
    from pb_bss_amd.distribution.utils import (get_trainer_class_from_model, parameter_from_dict,
                                               stack_parameters)
    y = oc.frames(4, (2, 30, 3))
    models = [dist.ComplexCircularSymmetricGaussianTrainer().fit(y[i]) for i in range(2)]
    again = parameter_from_dict('ComplexCircularSymmetricGaussian', models[0].to_dict())
    assert isinstance(again, dist.ComplexCircularSymmetricGaussian)
    assert (again.covariance == models[0].covariance).all()
    assert get_trainer_class_from_model(again) is dist.ComplexCircularSymmetricGaussianTrainer
    stacked = stack_parameters(models)
    assert stacked.covariance.shape == (2, 3, 3)
    np.testing.assert_array_equal(stacked.log_pdf(y)[1], models[1].log_pdf(y[1]))


def test_sampling_and_argument_errors(dev):
    from pb_bss_amd.distribution import (ComplexCircularSymmetricGaussian,
                                         ComplexCircularSymmetricGaussianTrainer)
    model = ComplexCircularSymmetricGaussian(covariance=oc.sample_covariance())
    np.random.seed(oc.SAMPLE_SEED)
    assert (model.sample(oc.SAMPLE_SIZE) == oc.fixtures()['sample']).all()
    with pytest.raises(NotImplementedError):
        ComplexCircularSymmetricGaussian(covariance=np.stack([np.eye(3)] * 2)).sample((4,))
    y = oc.frames(4, (30, 3))
    with pytest.raises(AssertionError):
        ComplexCircularSymmetricGaussianTrainer().fit(y.real)
    with pytest.raises(AssertionError):
        model.log_pdf(oc.frames(4, (30, oc.SAMPLE_D)).real)
    with pytest.raises(ValueError, match='Unknown covariance type'):
        ComplexCircularSymmetricGaussianTrainer().fit(y, covariance_type='spherical')


def test_raw_c_abi_refuses_bad_shapes(dev):
    _lib, _ = dev
    t = _lib.torch()
    lib, h = _lib.load(), _lib.handle(0)
    y = t.zeros((1, 4, 40), dtype=t.complex128, device='cuda')
    cov = t.zeros((1, 1, 40, 40), dtype=t.complex128, device='cuda')
    lp = t.full((1, 1, 4), 7.0, dtype=t.float64, device='cuda')
    st = t.full((1, 1), 7, dtype=t.int32, device='cuda')
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    for D, N, want in ((0, 4, _lib.ERR_UNSUPPORTED), (35, 4, _lib.ERR_UNSUPPORTED),
                       (3, 0, _lib.ERR_INVALID_ARG)):
        assert lib.pbbss_ccsg_log_pdf(h, p(y), 1, 1, N, D, 1, p(cov), p(lp), None, p(st),
                                      None) == want
        assert lib.pbbss_ccsg_fit(h, p(y), 1, 1, N, D, 1, None, 0, 0.0, p(cov), None) == want
    assert lib.pbbss_ccsg_fit(h, p(y), 1, 1, 4, 3, 2, None, 0, 0.0, p(cov), None) == \
        _lib.ERR_INVALID_ARG  # two classes need a saliency
    t.cuda.synchronize()
    assert bool((lp == 7.0).all()) and bool((st == 7).all()) and bool((cov == 0).all())
