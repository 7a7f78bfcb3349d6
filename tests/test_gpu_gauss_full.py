"""GPU: the full-covariance Gaussian kernels (csrc/gauss_full.hip: FP64-MFMA scatter, workgroup
Cholesky with inverse, MFMA log-pdf) at every compiled shape and on hard input, and the other
single-pass Gaussian M-steps where they used to centre on row 0 of the mixture.  Inputs and the
extended-precision reference: tests/oracle_gauss_full.py; that the float64 oracle may stand in for
it (1e-13 on every hard input): tests/test_gauss_full_oracle.py.  Everything goes through the
C ABI.

Tolerances are those of test_gaussian_full_covariance_against_oracle (mean atol 1e-11, covariance
1e-11 max|cov|, exact symmetry, log-pdf rtol 1e-9 / atol 1e-7, log-determinant rtol 1e-10) and,
for the mixture trainers, those of the oracle comparisons of tests/test_gpu_embed.py.  Where the
data are not of unit scale (rows at 1e6, rows times 1e+-100) the mean's tolerance is 1e-11 of
max|mean|: a mean at 1e6 is representable to 1e-10 only.

The log-pdf of an ill-conditioned covariance is no better than the float64 oracle itself.  Its
error against the longdouble restatement, relative to max|log_pdf| (measured on the CPU by
tests/test_gauss_full_oracle.py, which also checks this table against what it measures):

    cond(cov)   oracle log-pdf error / max|log_pdf|
    1e2         1.1e-15
    1e6         1.9e-12
    1e10        5.3e-08

The device's tolerance on such a case is the larger of the plain one and 32 x that figure: both
sides are backward-stable factorisations of the same float64 covariance that differ in
elimination and summation order, not in kind.
"""
import functools

import numpy as np
import pytest

import oracle_gauss_full as og
from oracle import embed as oe

pytestmark = pytest.mark.gpu

LOG_PDF_ORACLE_ERROR = {1e2: 1.1e-15, 1e6: 1.9e-12, 1e10: 5.3e-08}
DTYPES = (np.float32, np.float64)


def log_det_pc(cov):
    chol_inv = np.linalg.inv(np.linalg.cholesky(cov))
    return np.sum(np.log(np.diagonal(chol_inv, axis1=-2, axis2=-1)), -1)


def check_model(m, om, oc, what='', unit=1.0):
    """mean / covariance of a fit against the oracle's at the single-fit tolerances; `unit`: the
    scale of the mean where the data are not of unit scale."""
    scale = np.abs(oc).max()
    mtol = 1e-11 * unit
    print(f'{what}: mean err {np.abs(m.mean - om).max():.2e} (tol {mtol:.1e}), '
          f'cov err {np.abs(m.covariance - oc).max() / scale if scale else 0:.2e} max|cov|')
    np.testing.assert_allclose(m.mean, om, atol=mtol, rtol=0, err_msg=what)
    np.testing.assert_allclose(m.covariance, oc, atol=1e-11 * scale, rtol=0, err_msg=what)
    assert (m.covariance == np.swapaxes(m.covariance, -1, -2)).all(), what


def check_log_pdf(m, y, om, oc, what='', oracle_error=0.0):
    y64 = np.asarray(y, dtype=np.float64)
    ref = oe.gaussian_log_pdf(y64[None], om, oc, 'full')
    lp = m.log_pdf(y[None])
    extra = 32 * oracle_error * np.abs(ref).max()
    print(f'{what}: log-pdf err {np.abs(lp - ref).max():.2e}, max|lp| {np.abs(ref).max():.2e}, '
          f'extra tolerance {extra:.1e}')
    assert (np.abs(lp - ref) <= np.maximum(1e-7 + 1e-9 * np.abs(ref), extra)).all(), what
    if not oracle_error:  # a 1e-11 max|cov| change moves ln det by E 1e-11 cond(cov): well-conditioned only
        np.testing.assert_allclose(m.log_det_precision_cholesky, log_det_pc(oc), rtol=1e-10)


def fit_full(y, w):
    from pb_bss_amd.distribution import GaussianTrainer
    return GaussianTrainer().fit(y[None], saliency=np.array(w), covariance_type='full')


def mild_cloud(N, E, seed):
    """the cloud of test_gaussian_full_covariance_against_oracle: cond(cov) ~ 1e2, float32 values"""
    rng = np.random.default_rng([seed, N, E])
    A = 0.6 * np.eye(E) + 0.4 * rng.normal(size=(E, E)) / np.sqrt(E)
    return (rng.normal(size=(N, E)) @ A + rng.normal(size=E) * 3).astype(np.float32)


# ------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize('E', og.E_SWEEP)
def test_every_cholesky_variant_and_tile_count(E):
    """K = 2, N = 4 (E + 1) + 3: every Q = ceil(E (E + 1) / 512) of gf_chol_inverse on both sides
    of its boundaries, every tile count with E + 1 exact and one over, E < 5.  N = 4 is below
    E + 1 for all but E <= 3 and below one trip of the scatter: mean and covariance only."""
    K = 2
    for N in (4 * (E + 1) + 3, 4):
        y32 = mild_cloud(N, E, 1)
        w = np.random.default_rng([E, N]).uniform(size=(K, N)) ** 2
        for dtype in DTYPES:
            y = y32.astype(dtype)
            om, oc = oe.gaussian_fit(y.astype(np.float64)[None], w, 'full')
            m = fit_full(y, w)
            what = f'E {E} Q {og.chol_positions(E)} N {N} {np.dtype(dtype).name}'
            check_model(m, om, oc, what)
            if N > 4:
                check_log_pdf(m, y, om, oc, what)


@pytest.mark.parametrize('N', [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025])
def test_sample_counts_around_lane_groups_trips_and_chunks(N):
    """E = 3, K = 2: lane groups of 4 samples, trips of 16, the steps of gf_chunks (one more
    workgroup per 256 samples) and waves whose sample range is empty."""
    E, K = 3, 2
    y32 = mild_cloud(N, E, 2)
    w = np.random.default_rng(N).uniform(size=(K, N)) ** 2
    for dtype in DTYPES:
        y = y32.astype(dtype)
        om, oc = oe.gaussian_fit(y.astype(np.float64)[None], w, 'full')
        check_model(fit_full(y, w), om, oc, f'N {N} {np.dtype(dtype).name}')


@pytest.mark.parametrize('B,K,N,E', [(130, 2, 300, 5), (1, 1, 1025, 5)])
def test_batches_with_one_chunk_and_a_single_class(B, K, N, E):
    """B K >= 256: one chunk per class (gf_chunks); B K = 1: all chunks on one class."""
    from pb_bss_amd import _lib, engine
    from pb_bss_amd.distribution import Gaussian
    rng = np.random.default_rng(B + N)
    y32 = np.stack([mild_cloud(N, E, 10 + b) for b in range(B)])
    w = rng.uniform(size=(B, K, N)) ** 2
    for dtype in DTYPES:
        y = y32.astype(dtype)
        om, oc = oe.gaussian_fit(y.astype(np.float64)[:, None], w, 'full')
        mean, cov = (_lib.to_host(a) for a in engine.gauss_full_fit(_lib.to_device(y),
                                                                    _lib.to_device(w)))
        check_model(Gaussian(mean=mean, covariance=cov), om, oc, f'B {B} {np.dtype(dtype).name}')
        lp, st = engine.gauss_full_log_pdf(_lib.to_device(y), _lib.to_device(om),
                                           _lib.to_device(oc))
        assert int(st.item()) == 0
        ref = oe.gaussian_log_pdf(y.astype(np.float64)[:, None], om, oc, 'full')
        np.testing.assert_allclose(_lib.to_host(lp), ref, rtol=1e-9, atol=1e-7)


def drawn_model(E, K, seed):
    rng = np.random.default_rng([seed, E, K])
    A = rng.normal(size=(K, E, E)) / np.sqrt(E)
    return rng.normal(size=(K, E)), A @ np.swapaxes(A, -1, -2) + np.eye(E)


@pytest.mark.parametrize('K', [1, 8, 9, 10, 33, 64])
def test_log_pdf_sample_block_edges(K):
    """E = 4; N at the edges of a workgroup's sample block S = 64 min(8, 64 // K) and of a
    wave's group of 16 samples."""
    from pb_bss_amd.distribution import Gaussian
    E = 4
    S = og.logpdf_blocks(K)
    assert S == 64 * min(8, 64 // K)
    mean, cov = drawn_model(E, K, 3)
    model = Gaussian(mean=mean, covariance=cov)
    for N in (S - 1, S, S + 1, 15, 16, 17):
        y32 = mild_cloud(N, E, 4)
        for dtype in DTYPES:
            y = y32.astype(dtype)
            ref = oe.gaussian_log_pdf(y.astype(np.float64)[None], mean, cov, 'full')
            lp = model.log_pdf(y[None])
            assert lp.shape == (K, N)
            np.testing.assert_allclose(lp, ref, rtol=1e-9, atol=1e-7, err_msg=f'K {K} N {N}')


@pytest.mark.parametrize('E,K', [(47, 4), (47, 7), (63, 2), (63, 64), (31, 8), (31, 15), (15, 31),
                                 (15, 64)])
def test_log_pdf_class_passes_with_a_short_last_pass(E, K):
    """KC = 64 KiB / (P (P + 1) doubles) classes per LDS pass: 3 at P = 48 (K = 4, 7: last pass
    of 1), 1 at P = 64 (one class per pass, K = 64), 7 at P = 32 (K = 8, 15: last pass of 1),
    30 at P = 16 (K = 31: 1 left, K = 64: 4 left).  Covariances drawn as A A^T + I: no fit."""
    from pb_bss_amd.distribution import Gaussian
    N = 100
    mean, cov = drawn_model(E, K, 5)
    y32 = mild_cloud(N, E, 6)
    for dtype in DTYPES:
        y = y32.astype(dtype)
        ref = oe.gaussian_log_pdf(y.astype(np.float64)[None], mean, cov, 'full')
        lp = Gaussian(mean=mean, covariance=cov).log_pdf(y[None])
        np.testing.assert_allclose(lp, ref, rtol=1e-9, atol=1e-7)


def test_class_and_feature_bounds_are_refused():
    from pb_bss_amd import _lib, engine
    mean, cov = drawn_model(4, 65, 7)
    y = _lib.to_device(mild_cloud(20, 4, 7))[None]
    with pytest.raises(NotImplementedError):
        engine.gauss_full_log_pdf(y, _lib.to_device(mean)[None], _lib.to_device(cov)[None])
    y64 = mild_cloud(300, 64, 8)
    with pytest.raises(NotImplementedError):
        fit_full(y64, np.ones((2, 300)))
    mean, cov = drawn_model(64, 2, 9)
    with pytest.raises(NotImplementedError):
        engine.gauss_full_log_pdf(_lib.to_device(y64)[None], _lib.to_device(mean)[None],
                                  _lib.to_device(cov)[None])


# ------------------------------------------------------------------------------- hard input
DISTS = (1e2, 1e4, 1e6)
WEIGHTS = (0.0, 1e-12)


@pytest.mark.parametrize('weight', WEIGHTS)
@pytest.mark.parametrize('dist', DISTS)
def test_single_fit_with_row_0_off_centre(dist, weight):
    """The result must not depend on where a (nearly) weightless row lies: row 0 `dist` spreads
    from the cloud, and the same rows with the outlier moved to the end."""
    for dtype in DTYPES:
        models = []
        for where in ('first', 'last'):
            y64, w = og.off_centre(dist, weight, where)
            y = y64.astype(dtype)
            om, oc = oe.gaussian_fit(y.astype(np.float64)[None], w, 'full')
            m = fit_full(y, w)
            check_model(m, om, oc, f'dist {dist:g} weight {weight:g} {where} {np.dtype(dtype).name}')
            models.append(m)
        scale = np.abs(models[1].covariance).max()
        np.testing.assert_allclose(models[0].mean, models[1].mean, atol=1e-11, rtol=0)
        np.testing.assert_allclose(models[0].covariance, models[1].covariance, atol=1e-11 * scale,
                                   rtol=0)


def gmm_init(K, N, seed=11):
    init = np.random.default_rng(seed).uniform(size=(K, N))
    return init / init.sum(0)


def check_gmm(m, o, y, what):
    """tolerances of test_gmm_full_covariance_matches_reference_and_oracle (oracle part)"""
    y64 = np.asarray(y, dtype=np.float64)
    want = oe.gmm_predict(o, y64, 'full')
    got = m.predict(y)
    print(f'{what}: mean {np.abs(m.gaussian.mean - o["mean"]).max():.2e} '
          f'cov {np.abs(m.gaussian.covariance - o["covariance"]).max():.2e} '
          f'weight {np.abs(m.weight - o["weight"]).max():.2e} predict {np.abs(got - want).max():.2e}')
    np.testing.assert_allclose(m.gaussian.mean, o['mean'], atol=1e-8, err_msg=what)
    np.testing.assert_allclose(m.gaussian.covariance, o['covariance'], atol=1e-8, err_msg=what)
    np.testing.assert_allclose(m.weight, o['weight'], atol=1e-9, err_msg=what)
    np.testing.assert_allclose(got, want, atol=1e-6, err_msg=what)


@pytest.mark.parametrize('weight', WEIGHTS)
@pytest.mark.parametrize('dist', DISTS)
def test_gmm_full_with_row_0_off_centre(dist, weight):
    """GMMTrainer (default 'full'), 3 iterations: the first M-step has no previous mean."""
    from pb_bss_amd.distribution import GMMTrainer
    for dtype in DTYPES:
        models = []
        for where in ('first', 'last'):
            y64, w = og.off_centre(dist, weight, where)
            N = y64.shape[0]
            y = y64.astype(dtype)
            sal = np.ones(N)
            sal[0 if where == 'first' else -1] = weight
            init = gmm_init(2, N)
            if where == 'last':
                init = np.roll(init, -1, axis=1)
            o = oe.gmm_fit(y.astype(np.float64), init, 3, saliency=sal, covariance_type='full')
            m = GMMTrainer().fit(y, initialization=init, iterations=3, saliency=sal)
            check_gmm(m, o, y, f'dist {dist:g} weight {weight:g} {where} {np.dtype(dtype).name}')
            models.append(m)
        np.testing.assert_allclose(models[0].gaussian.mean, models[1].gaussian.mean, atol=1e-8)
        np.testing.assert_allclose(models[0].gaussian.covariance, models[1].gaussian.covariance,
                                   atol=1e-8)


@functools.lru_cache(maxsize=None)
def joint_case(dist, weight, shifted):
    """The smallest joint problem of tests/test_gpu_embed.py with the embedding of bin 0, frame 0
    `dist` spreads (0.35 / sqrt(E) per component) from the cloud and saliency[0, 0] = weight;
    `shifted`: frame 0 of every bin moved to the end, which no joint model can tell apart."""
    from oracle import synth
    Y, e, init = synth.make_joint(5, 90, 3, 2, 12, seed=2)
    e = e.astype(np.float64)
    u = np.random.default_rng(3).normal(size=12)
    u /= np.linalg.norm(u)
    e[0, 0] = e.reshape(-1, 12)[1:].mean(0) + dist * 0.35 / np.sqrt(12) * u
    sal = np.ones(Y.shape[:2])
    sal[0, 0] = weight
    if shifted:
        Y, e, sal = (np.roll(a, -1, axis=1) for a in (Y, e, sal))
        init = np.roll(init, -1, axis=2)
    return Y, e.astype(np.float32), init, sal


@pytest.mark.parametrize('weight', WEIGHTS)
@pytest.mark.parametrize('dist', DISTS)
@pytest.mark.parametrize('covariance_type', ['full', 'spherical'])
@pytest.mark.parametrize('iterations', [1, 3])
def test_gcacgmm_with_a_masked_outlier_at_bin_0_frame_0(iterations, covariance_type, dist, weight):
    """Row 0 of the joint models' (F T, E) embedding is bin 0, frame 0: what `saliency` exists to
    mask.  Tolerances of test_gcacgmm_full_config5_shape_against_oracle."""
    from pb_bss_amd.distribution import GCACGMMTrainer
    models = []
    for shifted in (False, True):
        Y, e, init, sal = joint_case(dist, weight, shifted)
        Y128, e64 = Y.astype(np.complex128), e.astype(np.float64)
        ref = oe.joint_fit('gaussian', Y128, e64, init, iterations, saliency=sal,
                           covariance_type=covariance_type)
        for dtype in DTYPES:
            model = GCACGMMTrainer().fit(Y, e.astype(dtype), initialization=init,
                                         iterations=iterations, saliency=sal,
                                         covariance_type=covariance_type)
            aff = model.predict(Y, e.astype(dtype))
            want = oe.joint_model_predict(ref, Y128, e64)
            what = f'{covariance_type} it {iterations} dist {dist:g} weight {weight:g} shifted {shifted}'
            print(f'{what}: mean {np.abs(model.gaussian.mean - ref["mean"]).max():.2e} '
                  f'cov {np.abs(model.gaussian.covariance / ref["covariance"] - 1).max():.2e} '
                  f'aff {np.abs(aff - want).max():.2e}')
            np.testing.assert_allclose(model.gaussian.mean, ref['mean'], atol=1e-8, err_msg=what)
            np.testing.assert_allclose(model.gaussian.covariance, ref['covariance'], rtol=1e-6,
                                       atol=1e-9, err_msg=what)
            assert np.abs(aff - want).max() < 1e-6, what
        models.append(model)
    np.testing.assert_allclose(models[0].gaussian.mean, models[1].gaussian.mean, atol=1e-8)
    np.testing.assert_allclose(models[0].gaussian.covariance, models[1].gaussian.covariance,
                               rtol=1e-6, atol=1e-9)


@pytest.fixture
def world1_nccl():
    """as tests/test_gpu_comm.py: the collectives of a sharded fit really enqueued, at world size 1"""
    import os
    import torch
    import torch.distributed as dist
    from pb_bss_amd import sharding
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29534')
    created = not dist.is_initialized()
    if created:
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
    sharding.init_native_comm()
    try:
        yield
    finally:
        sharding.destroy_native_comm()
        if created:
            dist.destroy_process_group()


@pytest.mark.parametrize('weight', WEIGHTS)
@pytest.mark.parametrize('dist', DISTS)
@pytest.mark.parametrize('iterations', [1, 3])
def test_sharded_gcacgmm_full_with_a_masked_outlier(world1_nccl, iterations, dist, weight):
    """Bins sharded over ranks: one centre common to all ranks in the first M-step (the all-reduced
    column mean, which the outlier moves by dist / (F T) spreads), the previous means after it.
    Masks at the tolerance of test_sharded_joint_fit_world1_equals_oracle."""
    from pb_bss_amd import _lib, sharding
    from pb_bss_amd.distribution import GCACGMMTrainer, _joint
    Y, e, init, sal = joint_case(dist, weight, False)
    real = _joint.sharded_bins
    _joint.sharded_bins = lambda enabled=True: real(True)  # world size 1 would skip the collective
    try:
        masks = sharding.fit_predict_sharded_joint(GCACGMMTrainer(), Y, e, np.array(init),
                                                   iterations=iterations, saliency=np.array(sal),
                                                   covariance_type='full')
    finally:
        _joint.sharded_bins = real
    Y128, e64 = Y.astype(np.complex128), e.astype(np.float64)
    ref = oe.joint_fit('gaussian', Y128, e64, init, iterations, saliency=sal, covariance_type='full')
    err = np.abs(_lib.to_host(masks) - oe.joint_model_predict(ref, Y128, e64)).max()
    print(f'sharded full it {iterations} dist {dist:g} weight {weight:g}: masks {err:.2e}')
    assert err < 1e-6


@functools.lru_cache(maxsize=None)
def wide_case(dist, weight, where):
    """Twelve clusters as tests/test_gpu_embed_wide.py draws them (N, E, K = 3001, 12, 12), one
    row `dist` noise levels from the centre of the data with saliency `weight`."""
    N, E, K, noise = 3001, 12, 12, 0.5
    rng = np.random.default_rng(N + K)
    mu = rng.standard_normal((K, E)) * 2.0
    lab = rng.integers(K, size=N)
    y = mu[lab] + noise * rng.standard_normal((N, E))
    init = rng.uniform(size=(K, N)) + 2.0 * (np.arange(K)[:, None] == lab[None, :])
    init /= init.sum(0)
    sal = rng.uniform(0.1, 1.0, size=N)
    u = rng.standard_normal(E)
    y[0] = y[1:].mean(0) + dist * noise * u / np.linalg.norm(u)
    sal[0] = weight
    if where == 'last':
        y, sal, init = np.roll(y, -1, 0), np.roll(sal, -1), np.roll(init, -1, 1)
    return _frozen(y.astype(np.float32), init, sal)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.mark.parametrize('weight', WEIGHTS)
@pytest.mark.parametrize('dist', DISTS)
@pytest.mark.parametrize('covariance_type,iterations', [('spherical', 6), ('diagonal', 4)])
def test_wide_gmm_with_row_0_off_centre(covariance_type, iterations, dist, weight):
    """K = 12 runs on the class tiles of csrc/embed_wide.hip, whose shifted row tile is shared by
    all classes: one shift per mixture, which must not be a row that saliency masks.  Tolerances of
    test_gmm_spherical_wide_shapes_against_oracle / test_gmm_diagonal_wide_shapes_against_oracle."""
    from pb_bss_amd.distribution import GMMTrainer
    ptol = 1e-7 if covariance_type == 'spherical' else 1e-8
    models = []
    for where in ('first', 'last'):
        y32, init, sal = wide_case(dist, weight, where)
        y64 = y32.astype(np.float64)
        o = oe.gmm_fit(y64, init, iterations, saliency=sal, covariance_type=covariance_type)
        want = oe.gmm_predict(o, y64, covariance_type)
        for dtype in DTYPES:
            y = y32.astype(dtype)
            m = GMMTrainer().fit(y, initialization=np.array(init), iterations=iterations,
                                 saliency=np.array(sal), covariance_type=covariance_type)
            got = m.predict(y)
            what = f'{covariance_type} dist {dist:g} weight {weight:g} {where} {np.dtype(dtype).name}'
            print(f'{what}: mean {np.abs(m.gaussian.mean - o["mean"]).max():.2e} '
                  f'cov rel {np.abs(m.gaussian.covariance / o["covariance"] - 1).max():.2e} '
                  f'weight {np.abs(np.asarray(m.weight) - o["weight"]).max():.2e} '
                  f'predict {np.abs(got - want).max():.2e}')
            np.testing.assert_allclose(m.gaussian.mean, o['mean'], atol=1e-9, rtol=0, err_msg=what)
            if covariance_type == 'spherical':
                np.testing.assert_allclose(m.gaussian.covariance, o['covariance'], rtol=1e-9)
            else:
                assert np.abs(m.gaussian.covariance - o['covariance']).max() < 1e-9, what
            np.testing.assert_allclose(np.asarray(m.weight), o['weight'], atol=1e-10, rtol=0)
            assert np.abs(got - want).max() < ptol, what
        models.append(m)
    np.testing.assert_allclose(models[0].gaussian.mean, models[1].gaussian.mean, atol=1e-9, rtol=0)
    np.testing.assert_allclose(models[0].gaussian.covariance, models[1].gaussian.covariance,
                               rtol=1e-9, atol=1e-9 if covariance_type == 'diagonal' else 0)


@pytest.mark.parametrize('delta', [1e2, 1e4])
def test_separated_clusters(delta):
    """Two classes on clusters `delta` spreads apart: no common shift lies within both spreads.
    The single fit, and GMMTrainer started from the true labels."""
    from pb_bss_amd.distribution import GMMTrainer
    y64, w, lab = og.separated(delta)
    init = (lab[None, :] == np.arange(2)[:, None]).astype(np.float64)
    for dtype in DTYPES:
        y = y64.astype(dtype)
        yr = y.astype(np.float64)
        om, oc = oe.gaussian_fit(yr[None], w, 'full')
        check_model(fit_full(y, w), om, oc, f'delta {delta:g} {np.dtype(dtype).name}')
        o = oe.gmm_fit(yr, init, 3, covariance_type='full')
        m = GMMTrainer().fit(y, initialization=init, iterations=3)
        check_gmm(m, o, y, f'gmm delta {delta:g} {np.dtype(dtype).name}')


def test_rows_at_a_large_offset():
    y64, w = og.offset()
    for dtype in DTYPES:
        y = y64.astype(dtype)
        om, oc = oe.gaussian_fit(y.astype(np.float64)[None], w, 'full')
        m = fit_full(y, w)
        check_model(m, om, oc, f'offset {np.dtype(dtype).name}', unit=np.abs(om).max())
        check_log_pdf(m, y, om, oc, f'offset {np.dtype(dtype).name}')


@pytest.mark.parametrize('factor', [1e100, 1e-100])
def test_rows_of_extreme_scale(factor):
    y, w = og.scaled(factor)
    om, oc = oe.gaussian_fit(y[None], w, 'full')
    check_model(fit_full(y, w), om, oc, f'scale {factor:g}', unit=np.abs(om).max())


@pytest.mark.parametrize('cond', [1e6, 1e10])
def test_ill_conditioned_covariance(cond):
    y64, w = og.conditioned(cond)
    for dtype in DTYPES:
        y = y64.astype(dtype)
        om, oc = oe.gaussian_fit(y.astype(np.float64)[None], w, 'full')
        m = fit_full(y, w)
        check_model(m, om, oc, f'cond {cond:g} {np.dtype(dtype).name}')
        check_log_pdf(m, y, om, oc, f'cond {cond:g} {np.dtype(dtype).name}',
                      oracle_error=LOG_PDF_ORACLE_ERROR[cond])


@pytest.mark.parametrize('delta', [1e3, 1e6])
def test_log_pdf_with_class_0_far_from_the_data(delta):
    """gf_logpdf_kernel shifts every row by the mean of class 0.  Class 1 sits on the data; its
    log-pdf against the oracle and against the same class evaluated alone."""
    from pb_bss_amd.distribution import Gaussian
    y64, w = og.conditioned(1e2)
    om, oc = oe.gaussian_fit(y64[None], w[:1], 'full')
    u = np.random.default_rng(12).normal(size=y64.shape[1])
    u /= np.linalg.norm(u)
    mean = np.concatenate([om + delta * u, om])
    cov = np.concatenate([oc, oc])
    for dtype in DTYPES:
        y = y64.astype(dtype)
        ref = oe.gaussian_log_pdf(y.astype(np.float64)[None], mean, cov, 'full')
        lp = Gaussian(mean=mean, covariance=cov).log_pdf(y[None])
        alone = Gaussian(mean=mean[1:], covariance=cov[1:]).log_pdf(y[None])
        print(f'delta {delta:g} {np.dtype(dtype).name}: near class err {np.abs(lp[1] - ref[1]).max():.2e}, '
              f'against itself alone {np.abs(lp[1] - alone[0]).max():.2e}')
        np.testing.assert_allclose(lp[1], ref[1], rtol=1e-9, atol=1e-7)
        np.testing.assert_allclose(lp[1], alone[0], rtol=1e-9, atol=1e-7)


def test_empty_class():
    """sum w = 0: the reference's 0 / tiny is mean 0 and covariance 0, not row 0 of the data."""
    from pb_bss_amd.distribution import GMMTrainer
    y64, w = og.empty_class()
    for dtype in DTYPES:
        y = y64.astype(dtype)
        om, oc = oe.gaussian_fit(y.astype(np.float64)[None], w, 'full')
        m = fit_full(y, w)
        check_model(m, om, oc, f'empty {np.dtype(dtype).name}')
        assert (m.mean[1] == 0).all() and (m.covariance[1] == 0).all()
        init = gmm_init(2, y.shape[0])
        init[1] = 0.0
        with pytest.raises(ValueError, match='ill-defined'):
            GMMTrainer().fit(y, initialization=init, iterations=2)


@pytest.mark.parametrize('row', [0, 137])
def test_nan_in_a_weightless_row(row):
    """0 * NaN is NaN in the reference's einsum: compared for NaN-ness only."""
    from pb_bss_amd.distribution import GMMTrainer
    y64, w = og.nan_row(row)
    for dtype in DTYPES:
        y = y64.astype(dtype)
        om, oc = oe.gaussian_fit(y.astype(np.float64)[None], w, 'full')
        m = fit_full(y, w)
        assert (np.isnan(m.mean) == np.isnan(om)).all()
        assert (np.isnan(m.covariance) == np.isnan(oc)).all()
        sal = np.ones(y.shape[0])
        sal[row] = 0.0
        with pytest.raises(ValueError, match='ill-defined'):
            GMMTrainer().fit(y, initialization=gmm_init(2, y.shape[0]), iterations=2, saliency=sal)
