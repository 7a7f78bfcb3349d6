"""CPU: the committed golden fixtures are what the UNMODIFIED reference produces, and the NumPy
oracle agrees with the reference on freshly drawn inputs -- i.e. the pin of the oracle can be
re-derived, not just trusted.  The reference's outputs on these inputs are stored in
tests/golden/reference_live.npz and reference_live_gev.npz, recorded from the reference itself
(imported through oracle/refshim.py) by `python -m oracle.make_golden live`
and `... live_gev`; the inputs are rebuilt here from the same seeds."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def ref():
    with np.load(os.path.join(GOLDEN, 'reference_live.npz')) as g:
        return {k: g[k] for k in g.files}


def test_committed_fixture_equals_live_reference(ref):
    g = np.load(os.path.join(GOLDEN, 'cacgmm_f9_t120_d8_k3.npz'))
    np.testing.assert_allclose(ref['fixture_cacgmm_affiliation'], g['affiliation'], atol=1e-12)
    g = np.load(os.path.join(GOLDEN, 'beamformer_extra_f19_d5.npz'))
    np.testing.assert_allclose(ref['fixture_lcmv_10'], g['lcmv_10'], atol=1e-12)
    np.testing.assert_allclose(ref['fixture_phase_3d'], g['phase_3d'], atol=1e-14)


def test_oracle_equals_live_reference_on_fresh_inputs(ref):
    from oracle import beamformer as ob, cacgmm as oc, embed as oe, permutation_alignment as op, synth
    Y, e, init = synth.make_joint(7, 90, 5, 2, 8, seed=1234)
    Y128, e64 = Y.astype(np.complex128), e.astype(np.float64)
    o = oc.em_fit(Y128, init, iterations=6)
    np.testing.assert_allclose(oc.em_predict(o, Y128), ref['cacgmm_masks'], atol=1e-10)
    oj = oe.joint_fit('gaussian', Y128, e64, init, 4)
    np.testing.assert_allclose(oe.joint_model_predict(oj, Y128, e64), ref['gcacgmm_masks'],
                               atol=1e-10)
    masks = ref['cacgmm_masks']
    X = Y128.transpose(0, 2, 1)
    psd = ref['psd']
    np.testing.assert_allclose(ob.psd(X, masks), psd, atol=1e-13)
    np.testing.assert_allclose(ob.mvdr_souden(psd[:, 0], psd[:, 1], ref_channel=0),
                               ref['mvdr_souden'], atol=1e-12)
    kft = np.ascontiguousarray(masks.transpose(1, 0, 2))
    np.testing.assert_array_equal(op.dhtv_calculate_mapping(kft, ref['dhtv_plan']),
                                  ref['dhtv_mapping'])
    for metric in ('cos', 'multiply', 'euclidean'):
        np.testing.assert_array_equal(op.greedy_calculate_mapping(kft, metric),
                                      ref[f'greedy_{metric}'])
        shuffled = np.ascontiguousarray(kft[::-1])
        for alg in ('greedy', 'optimal'):
            np.testing.assert_array_equal(
                op.oracle_calculate_mapping(shuffled, kft, metric, alg),
                ref[f'oracle_{metric}_{alg}'])


def test_oracle_gmm_equals_live_reference_on_fresh_inputs(ref):
    """GMMTrainer (covariance_type 'full' -- its default -- and 'spherical') and the Gaussian
    single fits of the unmodified reference against the NumPy oracle on freshly drawn data."""
    from oracle import embed as oe
    rng = np.random.default_rng(4321)
    N, E, K = 700, 9, 3
    centers = rng.normal(size=(K, E)) * 2
    y = centers[rng.integers(K, size=N)] + rng.normal(size=(N, E))
    init = rng.uniform(size=(K, N))
    init /= init.sum(0, keepdims=True)
    sal = rng.uniform(0.2, 1.0, size=N)
    for ct in ('full', 'spherical'):
        o = oe.gmm_fit(y, init, 5, saliency=sal, covariance_type=ct)
        np.testing.assert_allclose(o['mean'], ref[f'gmm_{ct}_mean'], atol=1e-11)
        np.testing.assert_allclose(o['covariance'], ref[f'gmm_{ct}_covariance'], atol=1e-11)
        np.testing.assert_allclose(o['weight'], ref[f'gmm_{ct}_weight'], atol=1e-12)
        np.testing.assert_allclose(oe.gmm_predict(o, y, ct), ref[f'gmm_{ct}_predict'], atol=1e-10)
    w = rng.uniform(size=(K, N))
    om, oc = oe.gaussian_fit(y[None], w, 'full')
    np.testing.assert_allclose(om, ref['gaussian_mean'], atol=1e-12)
    np.testing.assert_allclose(oc, ref['gaussian_covariance'], atol=1e-12)
    np.testing.assert_allclose(oe.gaussian_log_pdf(y[None], om, oc, 'full'),
                               ref['gaussian_log_pdf'], rtol=1e-10, atol=1e-9)


def test_oracle_mixture_weight_axes_equal_live_reference(ref):
    """The options the step-wise device loop serves (tests/test_gpu_embed_stepwise.py compares it
    with the oracle): weight_constant_axis sets over an independent axis for VMFMM / GMM and
    covariance_type='diagonal' -- oracle == unmodified reference on fresh inputs."""
    from oracle import embed as oe
    rng = np.random.default_rng(11)
    y = rng.standard_normal((3, 120, 5)) + rng.integers(0, 3, size=(3, 120, 1)) * 2.0
    init = rng.uniform(size=(3, 3, 120))
    init /= init.sum(axis=1, keepdims=True)
    sal = rng.uniform(0.2, 1.0, size=(3, 120))
    for i, axis in enumerate(((-3,), (-3, -1))):
        o = oe.vmfmm_fit(y, init, iterations=3, saliency=sal, weight_constant_axis=axis)
        assert np.abs(ref[f'axes{i}_vmfmm_weight'] - o['weight']).max() < 1e-12
        assert np.abs(ref[f'axes{i}_vmfmm_mean'] - o['mean']).max() < 1e-12
        # SphericalGaussian.log_pdf does not broadcast over independent axes in the reference
        # (gaussian.py:110-113): 'spherical' is pinned on flat data only
        og = oe.gmm_fit(y, init, iterations=3, saliency=sal, weight_constant_axis=axis,
                        covariance_type='full')
        assert np.abs(ref[f'axes{i}_gmm_weight'] - og['weight']).max() < 1e-12
        assert np.abs(ref[f'axes{i}_gmm_covariance'] - og['covariance']).max() < 1e-10
    for i, axis in enumerate(((-1,), (-2,), -2)):
        og = oe.gmm_fit(y[0], init[0], iterations=3, saliency=sal[0], weight_constant_axis=axis,
                        covariance_type='diagonal')
        assert np.abs(ref[f'diag{i}_mean'] - og['mean']).max() < 1e-12
        assert np.abs(ref[f'diag{i}_covariance'] - og['covariance']).max() < 1e-12
        assert np.abs(ref[f'diag{i}_predict'] - oe.gmm_predict(og, y[0], 'diagonal')).max() < 1e-10


def test_gev_use_eig_fixture_equals_reference_cython_modules():
    """The reference's two native files (extraction/cythonized/c_eig.pyx: zggev, behind
    `get_gev_vector(use_eig=True)`; get_gev_vector.pyx: zhegvd, the default path), compiled out
    of tree by oracle/refshim.py:build_cython: the committed fixture is what they produce, and
    the oracle agrees with them on fresh pencils."""
    from oracle import beamformer as ob
    g = np.load(os.path.join(GOLDEN, 'gev_use_eig.npz'))
    r = np.load(os.path.join(GOLDEN, 'reference_live_gev.npz'))

    def cos(a, b):
        return np.abs((a.conj() * b).sum(-1)) / np.linalg.norm(a, axis=-1) / np.linalg.norm(b, axis=-1)
    for tag in ('hpd_d6', 'indef_d5', 'general_d6'):
        assert np.abs(cos(r[tag + '_w'], g[tag + '_w_cython']) - 1).max() < 1e-12, tag
    rng = np.random.default_rng(99)
    A = rng.standard_normal((6, 5, 5)) + 1j * rng.standard_normal((6, 5, 5))
    B = rng.standard_normal((6, 5, 5)) + 1j * rng.standard_normal((6, 5, 5)) + 2 * np.eye(5)
    assert np.abs(cos(r['general_w_eig'], ob.gev_vector_eig(A, B)) - 1).max() < 1e-12
    X = rng.standard_normal((6, 5, 20)) + 1j * rng.standard_normal((6, 5, 20))
    P = X @ X.conj().swapaxes(-1, -2)
    Q = P + np.eye(5)
    assert np.abs(cos(r['hpd_w_zhegvd'], ob.gev_vector(P, Q)) - 1).max() < 1e-12
