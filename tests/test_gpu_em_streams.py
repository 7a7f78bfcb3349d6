"""The instruction streams of the cACGMM EM kernel's E and M phases, at the smallest shapes that
reach what they can get wrong (csrc/cacgmm_em.hpp phase_e / phase_m, csrc/pbbss_dev.hpp butterflies).

* M phase: every wave's accumulators go through the halving butterfly (DPP exchanges without an
  `old` operand) and the write-back table; a wrong exchange or destination shows up as a swapped,
  conjugated or partial ENTRY of the covariance, which mask-level tests can hide -- so the
  K x D x D covariance of one stand-alone M-step is compared entry by entry.
* E phase: frame validity rides on the saliency factor (`salm`), the class exponents are kept with
  the sign flipped (`emin - nex`), the activity mask is applied after the class loop.

Tolerances are the ones of tests/test_gpu_em.py for the same quantities (single M-step 1e-12,
predict: q 1e-11 relative to max q, affiliation 1e-10; two iterations: masks 1e-7, weights 1e-8),
except where the docstring of a test derives another one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    from pb_bss_amd import _lib
    return _lib.to_device(x, dtype)


def _host(x):
    from pb_bss_amd import _lib
    return _lib.to_host(x)


def _cov(vec, val):
    return np.einsum('...wx,...x,...zx->...wz', vec, val, vec.conj())


@pytest.mark.parametrize('D,K', [(8, 2), (8, 3), (8, 4), (7, 3)])
def test_m_step_covariance_entry_by_entry(D, K):
    """F = 3, T = 65: two chunks of 64 frames, 63 padding frames in the second.  K = 2, 3, 4 pad
    the 16 slots per class to 32, 48 and 64 accumulators; D = 7 takes the round-robin entry map."""
    from oracle import synth, cacgmm as oc
    from pb_bss_amd import engine, _lib
    F, T = 3, 65
    Y, _ = synth.make_stft(F, T, D, 2, seed=10 * D + K)
    # the device keeps complex64 frames: the oracle gets the exact upcast of the same values
    yn = oc.normalize_observation(Y.astype(np.complex128)).astype(np.complex64)
    yn128 = yn.astype(np.complex128)
    rng = np.random.default_rng(K)
    aff = rng.uniform(0.05, 1.0, size=(F, K, T))
    aff /= aff.sum(axis=1, keepdims=True)
    q = rng.uniform(0.5, 2.0, size=(F, K, T))
    vec, val = oc.cacg_m_step(yn128[..., None, :, :], aff, q)
    want = D * np.einsum('fdn,fen,fkn->fkde', yn128, yn128.conj(), aff / q)
    want /= aff.sum(-1)[..., None, None]
    want = oc.force_hermitian(want)
    d_vec, d_val, d_cov, st = engine.cacg_m_step(_dev(yn), _dev(aff), _dev(q),
                                                 layout=_lib.LAYOUT_DT, want_cov=True)
    got = _host(d_cov)
    err = np.abs(got - want)
    print(f'D={D} K={K}: covariance max entry error {err.max():.2e}')
    assert err.max() < 1e-12, np.argwhere(err >= 1e-12)[:8]
    assert np.abs(_cov(_host(d_vec), _host(d_val)) - _cov(vec, val)).max() < 1e-12
    assert np.abs(_host(d_val) - val).max() < 1e-12


@pytest.fixture(scope='module')
def validity_data():
    """One observation; the three frame counts are prefixes of it."""
    from oracle import synth
    Y, init = synth.make_stft(3, 257, 8, 3, seed=41)
    sal = np.random.default_rng(5).uniform(0.1, 1.0, size=(3, 257))
    sal[:, ::5] = 0.0
    return Y, init, sal


@pytest.mark.parametrize('with_saliency', [False, True])
@pytest.mark.parametrize('T', [1, 64, 257])
def test_frame_validity_factor(validity_data, T, with_saliency):
    """T = 1 (one valid lane, 63 padding frames), 64 (no padding), 257 (a full pass of 256 frames
    plus one frame in the next): padding frames must add nothing to the class sums -- which reach
    the output through the mixture weights, in saliency mode normalised by their total -- nor to
    the covariance.  Two iterations against the oracle.

    T = 1 makes every covariance D y y^H: rank one, seven eigenvalues on the floor of 1e-10.  As in
    test_rank_deficient_hits_floor, B^-1 then carries entries of 1e10 (both sides form it before
    the quadratic form), and q ~ 1 is what is left of D^2 = 64 terms of that size: a rounding error
    of up to 1e10 * 1.1e-16 * 64 = 7e-5 in q, D times that, 6e-4, in the log-pdf and so at most in
    a posterior -- and in the weights, their mean over the one frame.  Hence that test's 1e-3 for
    T = 1; T >= 64 has full-rank covariances and the two-iteration tolerances."""
    from oracle import cacgmm as oc
    from pb_bss_amd import engine
    Y, init, sal = validity_data
    Y = np.ascontiguousarray(Y[:, :T])
    init = init[:, :, :T] / init[:, :, :T].sum(axis=1, keepdims=True)
    kw_o, kw_d = {}, {}
    if with_saliency:
        s = np.ascontiguousarray(sal[:, :T])
        if T == 1:
            s = np.full((3, 1), 0.7)
        kw_o, kw_d = dict(saliency=s), dict(saliency=_dev(s))
    Y128 = Y.astype(np.complex128)
    m = oc.em_fit(Y128, init, iterations=2, **kw_o)
    want = oc.em_predict(m, Y128)
    r = engine.em_fit(_dev(Y), 3, gamma0=_dev(init), iterations=2, final_predict=True, **kw_d)
    e_mask = np.abs(_host(r['affiliation']) - want).max()
    e_w = np.abs(_host(r['weight'])[..., None] - m['weight']).max()
    print(f'T={T} saliency={with_saliency}: mask error {e_mask:.2e}, weight error {e_w:.2e}')
    tol_mask, tol_w = (1e-3, 1e-3) if T == 1 else (1e-7, 1e-8)
    assert e_mask < tol_mask
    assert e_w < tol_w


def test_predict_over_the_exponent_range():
    """One E-step with q and the class determinants far apart in exponent: a bin scaled by 1e-18
    and one by 1e+18 in float32 (the kernel normalises the frames), an all-zero frame (q floored
    at `tiny`: the smallest exponent the softmax sees), and a model whose classes have
    determinants 1, 1e-16 and 1e-36 (on the zero frame the posteriors are exactly their ratio:
    1e-36, 1e-20, 1), so that the shifts `emin - nex[k]` of the softmax run from 0 to a few
    hundred binary orders."""
    from oracle import synth, cacgmm as oc
    from pb_bss_amd import engine
    F, T, D, K = 3, 70, 8, 3
    Y, _ = synth.make_stft(F, T, D, K, seed=23)
    Y = Y.astype(np.complex64)
    Y[0] *= np.float32(1e-18)
    Y[1] *= np.float32(1e18)
    Y[2, 5] = 0
    Y[0, 69] = 0
    assert np.isfinite(Y).all() and (np.abs(Y[0, 0]) > 0).all()
    rng = np.random.default_rng(2)
    vec = np.linalg.qr(rng.standard_normal((F, K, D, D)) + 1j * rng.standard_normal((F, K, D, D)))[0]
    val = np.empty((F, K, D))
    val[:, 0] = 1.0
    val[:, 1] = np.logspace(0, -4, D)[::-1] * 1.0    # det 1e-16
    val[:, 2] = np.logspace(0, -9, D)[::-1] * 1.0    # det 1e-36, condition 1e9
    weight = np.full((F, K), 1.0 / K)
    model = dict(weight=weight[..., None], eigvec=vec, eigval=val)
    aff, q = oc.em_predict(model, Y.astype(np.complex128), return_quadratic_form=True)
    d_aff, d_q, _ = engine.em_predict(_dev(Y), _dev(vec), _dev(val), _dev(weight), want_q=True)
    e_q = np.abs(_host(d_q) - q).max() / q.max()
    e_a = np.abs(_host(d_aff) - aff).max()
    print(f'q error / max q {e_q:.2e}, affiliation error {e_a:.2e}')
    assert np.isfinite(_host(d_aff)).all()
    assert e_q < 1e-11
    assert e_a < 1e-10
    # the floored frames: q is exactly `tiny` for every class on both sides
    assert (_host(d_q)[2, :, 5] == np.finfo(np.float64).tiny).all()
    assert (q[2, :, 5] == np.finfo(np.float64).tiny).all()
