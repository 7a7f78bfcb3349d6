"""GPU: the frame-recursive cACGMM mask estimator (csrc/online_cacgmm.hip;
pb_bss_amd.distribution.recursive_cacgmm, OnlineCACGMM) against the NumPy restatement
tests/oracle_online_cacgmm.py.

E_CASE is the restatement's own error (float64 run against the longdouble run, relative to the
maximum of gamma, q, P, L (max(|L|, 1)), Lambda and pi) for exactly the inputs of the sweep, the
larger of both input dtypes; tests/test_online_cacgmm_oracle.py re-measures it and keeps this copy
within a factor of 4.  The device bound of a case is 16 * max(e_case, 1e-13) relative to the
maximum of the quantity, with the constants and the reasoning of tests/test_gpu_online_beamformer.py
and tests/test_gpu_wpe_online.py: the floor is about T eps for the longest row, 16 leaves room for
another summation order (the device adds its dot products on fixed lane trees and uses its own
series for the logarithm and the exponential).
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle_online_cacgmm as oc

pytestmark = pytest.mark.gpu

E_CASE = {
    ((2, 2, 64), 1.0): (1.4e-15, 1.3e-15, 1.1e-15, 7.2e-16, 4.0e-16, 4.5e-16),
    ((2, 2, 64), 0.999): (1.5e-15, 1.3e-15, 1.2e-15, 1.1e-15, 8.2e-16, 5.4e-16),
    ((2, 2, 64), 0.95): (1.8e-15, 1.8e-15, 3.0e-15, 8.4e-16, 1.0e-15, 1.1e-15),
    ((3, 2, 65), 1.0): (1.1e-15, 1.3e-15, 1.7e-15, 1.8e-15, 6.9e-16, 5.0e-16),
    ((3, 2, 65), 0.999): (1.8e-15, 3.3e-15, 2.2e-15, 1.7e-15, 7.1e-16, 5.9e-16),
    ((3, 2, 65), 0.95): (2.8e-15, 2.0e-15, 1.8e-15, 1.6e-15, 1.2e-15, 1.3e-15),
    ((4, 3, 130), 1.0): (5.5e-15, 4.7e-15, 5.3e-15, 3.6e-15, 1.2e-15, 1.1e-15),
    ((4, 3, 130), 0.999): (9.9e-15, 3.6e-15, 4.0e-15, 3.4e-15, 3.1e-15, 3.2e-15),
    ((4, 3, 130), 0.95): (2.8e-14, 1.4e-14, 1.6e-14, 1.3e-15, 7.1e-15, 7.2e-15),
    ((5, 4, 33), 1.0): (2.2e-15, 3.1e-15, 3.3e-15, 6.3e-16, 2.4e-16, 2.4e-16),
    ((5, 4, 33), 0.999): (1.8e-15, 1.6e-15, 2.0e-15, 9.4e-16, 4.9e-16, 3.2e-16),
    ((5, 4, 33), 0.95): (2.4e-15, 2.3e-15, 2.0e-15, 8.5e-16, 5.3e-16, 6.0e-16),
    ((8, 3, 300), 1.0): (2.2e-14, 9.1e-15, 1.1e-14, 3.5e-15, 1.7e-15, 1.2e-15),
    ((8, 3, 300), 0.999): (5.9e-15, 6.2e-15, 7.9e-15, 3.8e-15, 1.6e-15, 8.9e-16),
    ((8, 3, 300), 0.95): (1.3e-13, 2.7e-14, 2.4e-14, 3.1e-15, 1.3e-14, 1.3e-14),
    ((16, 8, 200), 1.0): (2.4e-14, 9.7e-15, 1.3e-14, 9.4e-15, 4.2e-15, 2.6e-15),
    ((16, 8, 200), 0.999): (1.3e-14, 1.1e-14, 1.1e-14, 4.6e-15, 5.2e-15, 2.2e-15),
    ((16, 8, 200), 0.95): (1.4e-13, 1.1e-14, 2.7e-14, 3.6e-15, 3.0e-14, 2.9e-14),
    ((2, 2, 1000), 1.0): (1.6e-14, 9.8e-15, 1.2e-14, 6.6e-15, 6.0e-15, 5.9e-15),
    ((2, 2, 1000), 0.999): (1.7e-14, 1.0e-14, 8.3e-15, 3.7e-15, 8.1e-15, 6.5e-15),
    ((2, 2, 1000), 0.95): (7.8e-14, 4.0e-14, 5.0e-14, 1.1e-14, 4.5e-14, 4.5e-14),
    ((2, 2, 31), 1.0): (1.1e-15, 1.0e-15, 8.5e-16, 8.4e-16, 4.6e-16, 5.8e-16),
    ((2, 2, 31), 0.999): (1.2e-15, 1.1e-15, 8.5e-16, 9.3e-16, 4.7e-16, 3.9e-16),
    ((2, 2, 31), 0.95): (6.9e-16, 1.2e-15, 1.1e-15, 1.6e-15, 8.8e-16, 7.8e-16),
    ((2, 2, 32), 1.0): (3.8e-15, 7.7e-16, 9.7e-16, 2.8e-15, 1.8e-15, 1.9e-15),
    ((2, 2, 32), 0.999): (1.0e-15, 3.8e-16, 5.8e-16, 2.4e-15, 8.4e-16, 7.4e-16),
    ((2, 2, 32), 0.95): (1.6e-15, 6.1e-16, 7.9e-16, 2.0e-15, 1.1e-15, 1.2e-15),
    ((2, 2, 33), 1.0): (8.1e-16, 6.2e-16, 7.3e-16, 1.2e-15, 4.2e-16, 4.6e-16),
    ((2, 2, 33), 0.999): (8.1e-16, 9.2e-16, 9.4e-16, 8.1e-16, 5.8e-16, 4.6e-16),
    ((2, 2, 33), 0.95): (1.3e-15, 7.8e-16, 9.7e-16, 1.1e-15, 7.2e-16, 8.2e-16),
    ((9, 3, 70), 1.0): (3.7e-15, 2.5e-15, 2.5e-15, 9.8e-16, 9.1e-16, 5.6e-16),
    ((9, 3, 70), 0.999): (5.6e-15, 1.5e-15, 2.1e-15, 1.7e-15, 8.3e-16, 5.6e-16),
    ((9, 3, 70), 0.95): (2.2e-14, 3.3e-15, 4.4e-15, 1.5e-15, 3.5e-15, 3.4e-15),
    ((12, 5, 70), 1.0): (7.3e-15, 2.2e-15, 3.6e-15, 2.3e-15, 7.3e-16, 6.3e-16),
    ((12, 5, 70), 0.999): (4.9e-15, 4.0e-15, 2.4e-15, 1.7e-15, 9.0e-16, 5.4e-16),
    ((12, 5, 70), 0.95): (1.0e-14, 3.3e-15, 3.6e-15, 1.2e-15, 6.5e-16, 5.4e-16),
    ((4, 8, 40), 1.0): (2.7e-15, 8.9e-16, 1.1e-15, 2.6e-15, 1.2e-15, 1.2e-15),
    ((4, 8, 40), 0.999): (2.6e-15, 9.8e-16, 9.5e-16, 1.1e-15, 7.1e-16, 6.7e-16),
    ((4, 8, 40), 0.95): (3.6e-15, 1.3e-15, 1.5e-15, 1.3e-15, 1.5e-15, 1.5e-15),
    ((8, 8, 40), 1.0): (4.2e-15, 1.8e-15, 2.6e-15, 7.4e-16, 6.3e-16, 6.0e-16),
    ((8, 8, 40), 0.999): (4.1e-15, 1.4e-15, 2.2e-15, 7.3e-16, 4.8e-16, 4.8e-16),
    ((8, 8, 40), 0.95): (3.6e-15, 3.3e-15, 2.8e-15, 9.0e-16, 8.5e-16, 9.3e-16),
}
EPS = 2.0 ** -52


@pytest.fixture(scope='module')
def dist():
    from pb_bss_amd import _lib
    from pb_bss_amd import distribution
    _lib.require_gpu()
    return distribution


@functools.lru_cache(maxsize=None)
def reference(case, alpha, dtype_name):
    """(Y (BATCH, D, T), initial state, B0, gamma, q, P, L, Lambda, pi) of the restatement."""
    Y, state, B0 = oc.case_input(case, np.dtype(dtype_name))
    out = oc.recursive(Y, state, alpha, oc.EPS_AFF)
    assert not out[6].any()
    out = (Y, state, B0) + out[:6]
    for a in (Y, B0) + state + out[3:]:
        a.setflags(write=False)
    return out


def host(a):
    return a.detach().cpu().numpy()


def same(a, b):
    """equal bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device_state(dist, state, rows=slice(None)):
    """an OnlineCACGMMState from the NumPy (P, L, Lambda, pi) of the problems `rows`"""
    from pb_bss_amd import _lib
    t = _lib.torch()
    P, L, Lam, pi = (t.from_numpy(np.array(a[rows])).cuda() for a in state)
    K, D = P.shape[-3:-1]
    return dist.OnlineCACGMMState(P.reshape(-1, K, D, D), L.reshape(-1, K), Lam.reshape(-1, K),
                                  pi.reshape(-1, K),
                                  t.zeros((P.reshape(-1, K, D, D).shape[0],), dtype=t.int64,
                                          device='cuda'))


def run(dist, Y, state, alpha, rows=slice(None), eps=oc.EPS_AFF, **kw):
    """recursive_cacgmm from the NumPy state -> (gamma, q, P, L, Lambda, pi, state)."""
    G, Q, st = dist.recursive_cacgmm(Y, None, alpha, affiliation_eps=eps,
                                     state=device_state(dist, state, rows), return_state=True,
                                     return_quadratic_form=True, **kw)
    G, Q = (a if isinstance(a, np.ndarray) else host(a) for a in (G, Q))
    return (G, Q, host(st.precision), host(st.log_determinant), host(st.count), host(st.weight),
            st)


@pytest.mark.parametrize('alpha', oc.ALPHAS)
@pytest.mark.parametrize('case', oc.CASES, ids=str)
def test_parity(dist, case, alpha):
    from pb_bss_amd import _lib
    t = _lib.torch()
    D, K, T = case
    worst = 0.0
    for dtype_name in ('complex128', 'complex64'):
        Y, state, _, *want = reference(case, alpha, dtype_name)
        for B in (1, oc.BATCH):
            rows = slice(0, B)
            for layout in (None, 'f t d'):
                if layout is None:
                    got = run(dist, Y[:B], state, alpha, rows)
                else:  # a non-contiguous (B, T, D) view of (B, D, T) memory
                    view = t.from_numpy(np.array(Y[:B])).cuda().transpose(1, 2)
                    assert not view.is_contiguous() or T == 1
                    got = run(dist, view, state, alpha, rows, layout=layout)
                G, Q, P, L, Lam, pi, st = got
                assert G.shape == Q.shape == (B, K, T) and P.shape == (B, K, D, D)
                assert L.shape == Lam.shape == pi.shape == (B, K)
                assert G.dtype == Q.dtype == L.dtype == np.float64 and P.dtype == np.complex128
                assert (host(st.frames_seen) == T).all() and (host(st.status) == 0).all()
                assert (P == P.conj().swapaxes(-1, -2)).all()       # Hermitian to the bit
                assert (np.diagonal(P, axis1=-2, axis2=-1).imag == 0).all()
                assert (Q[:, :, oc.zero_frame(case)] == 0).all()
                for name, have, ref, e in zip(oc.NAMES, got[:6], want, E_CASE[case, alpha]):
                    err, bound = oc.relative(have, ref[:B], name), 16 * max(e, 1e-13)
                    print(f'{case} a={alpha} {dtype_name} B={B} {layout} {name}: {err:.2e} '
                          f'(bound {bound:.2e})')
                    worst = max(worst, err / bound)
                    assert err <= bound, (case, alpha, dtype_name, B, layout, name, err, bound)
    print(f'{case} a={alpha}: worst {worst:.3f} of the bound')


@pytest.mark.parametrize('alpha', oc.ALPHAS)
@pytest.mark.parametrize('case', [(2, 2, 64), (4, 3, 130), (8, 3, 300), (12, 5, 70), (16, 8, 200),
                                  (2, 2, 1000)], ids=str)
def test_batch_route_on_the_devices_own_outputs(dist, case, alpha):
    """With the gamma and q that the device recorded, B_k is a plain weighted sum: P_k B_k = I
    within 16 cond eps, L_k = log det B_k within (16 + T) D eps of max(|L|, 1) (the bounds of
    tests/test_online_cacgmm_oracle.py)."""
    D, K, T = case
    Y, state, B0 = reference(case, alpha, 'complex128')[:3]
    G, Q, P, L, Lam, pi, _ = run(dist, Y, state, alpha)
    for b in range(oc.BATCH):
        Bk, Lk = oc.batch_covariance(Y[b], G[b], Q[b], alpha, B0[b], state[2][b])
        cond = np.linalg.cond(Bk)
        assert np.abs(Lam[b] - Lk).max() <= (16 + T) * EPS * np.abs(Lk).max()
        for k in range(K):
            err, tol = np.abs(P[b, k] @ Bk[k] - np.eye(D)).max(), 16 * cond[k] * EPS
            print(f'{case} a={alpha} b={b} k={k}: {err:.2e} (tol {tol:.2e}, cond {cond[k]:.1e})')
            assert err <= tol, (case, alpha, b, k, err, tol)
        want = np.linalg.slogdet(Bk)[1]
        err, tol = np.abs(L[b] - want).max(), (16 + T) * D * EPS * max(np.abs(want).max(), 1.0)
        assert err <= tol, (case, alpha, b, err, tol)


@pytest.mark.parametrize('case', [(2, 2, 130), (16, 3, 100), (8, 8, 70)], ids=str)
def test_blocking_is_bitwise_invisible(dist, case):
    from pb_bss_amd import _lib
    from pb_bss_amd.distribution import CACGMM, ComplexAngularCentralGaussian
    t = _lib.torch()
    D, K, T = case
    alpha = 0.95
    Y, state, B0 = oc.case_input(case, np.complex64)
    G, Q, P, L, Lam, pi, _ = run(dist, Y, state, alpha)

    def in_blocks(lengths):
        st, gs, qs, t0 = device_state(dist, state), [], [], 0
        for n in lengths:
            g, q, st = dist.recursive_cacgmm(Y[:, :, t0:t0 + n], None, alpha, state=st,
                                             return_state=True, return_quadratic_form=True)
            gs.append(g)
            qs.append(q)
            t0 += n
        assert t0 == T
        assert same(np.concatenate(gs, axis=-1), G) and same(np.concatenate(qs, axis=-1), Q)
        assert same(host(st.precision), P) and same(host(st.log_determinant), L)
        assert same(host(st.count), Lam) and same(host(st.weight), pi)
        assert (host(st.frames_seen) == T).all()
    in_blocks([1] * T)
    if T > 73:
        in_blocks([1, 1, 7, 64, T - 73])     # 9 + 64 straddles two tile edges
    in_blocks([31, 2, 31, T - 64])
    # OnlineCACGMM frame by frame and in blocks, in the (F, Tb, D) layout of OnlineWPE, from a
    # model whose state is the functional form's
    lam, vec = np.linalg.eigh(B0)
    model = CACGMM(weight=state[3][..., None], cacg=ComplexAngularCentralGaussian(vec, lam))
    first = dist.OnlineCACGMMState.from_model(model, oc.INITIAL_COUNT)
    want = dist.recursive_cacgmm(Y, model, alpha, initial_count=oc.INITIAL_COUNT,
                                 return_state=True, return_quadratic_form=True)
    by_frame = dist.OnlineCACGMM(model, alpha, initial_count=oc.INITIAL_COUNT)
    assert by_frame.status is None and same(host(by_frame.precision), host(first.precision))
    frames = [by_frame.step_frame(Y[:, :, i]) for i in range(T)]
    assert frames[0].shape == (oc.BATCH, K) and isinstance(frames[0], np.ndarray)
    assert same(np.stack(frames, axis=-1), want[0])
    by_block = dist.OnlineCACGMM(model, alpha, initial_count=oc.INITIAL_COUNT)
    Yd = t.from_numpy(np.ascontiguousarray(Y.swapaxes(1, 2))).cuda()       # (F, T, D)
    blocks = [by_block.step_block(Yd[:, a:b], return_quadratic_form=True)
              for a, b in ((0, 33), (33, 34), (34, T))]
    assert all(g.is_cuda and g.dtype == t.float64 for g, _ in blocks)
    assert same(host(t.cat([g for g, _ in blocks], dim=2)), want[0])
    assert same(host(t.cat([q for _, q in blocks], dim=2)), want[1])
    for o in (by_frame, by_block):
        assert same(host(o.precision), host(want[2].precision))
        assert same(host(o.log_determinant), host(want[2].log_determinant))
        assert same(host(o.count), host(want[2].count))
        assert same(host(o.weight), host(want[2].weight))
        assert (host(o.status) == 0).all()


def test_determinism_batch_independence_and_tensor_input(dist):
    from pb_bss_amd import _lib
    t = _lib.torch()
    case, alpha = (8, 3, 300), 0.999
    Y, state = reference(case, alpha, 'complex64')[:2]
    Y5 = np.concatenate([Y, Y[:2] * 0.5 + Y[1:] * 0.25])
    state5 = tuple(np.concatenate([a, a[:2]]) for a in state)
    a = run(dist, Y5, state5, alpha)
    again = run(dist, Y5, state5, alpha)
    assert all(same(a[i], again[i]) for i in range(6))
    for b in range(5):
        one = run(dist, Y5[b], state5, alpha, rows=b)
        assert one[0].shape == (3, 300) and one[2].shape == (1, 3, 8, 8)
        assert same(a[0][b], one[0]) and same(a[1][b], one[1]), b
        assert all(same(a[i][b], one[i][0]) for i in range(2, 6)), b
    # a tensor input gives what the NumPy input gives, as tensors, without a host synchronisation;
    # the passed state is not modified
    yd = t.from_numpy(Y5).cuda()
    std = device_state(dist, state5)
    keep = std.clone()
    t.cuda.synchronize()
    t.cuda.set_sync_debug_mode('error')
    try:
        gd, qd, st2 = dist.recursive_cacgmm(yd, None, alpha, state=std, return_state=True,
                                            return_quadratic_form=True)
    finally:
        t.cuda.set_sync_debug_mode('default')
    assert gd.is_cuda and qd.is_cuda and gd.dtype == qd.dtype == t.float64
    assert same(host(gd), a[0]) and same(host(qd), a[1]) and same(host(st2.precision), a[2])
    assert all(x.is_cuda for x in (st2.precision, st2.log_determinant, st2.count, st2.weight,
                                   st2.frames_seen, st2.status))
    assert st2.frames_seen.dtype == t.int64 and st2.status.dtype == t.int32
    for before, after in zip((keep.precision, keep.log_determinant, keep.count, keep.weight,
                              keep.frames_seen),
                             (std.precision, std.log_determinant, std.count, std.weight,
                              std.frames_seen)):
        assert bool((before == after).all())
    assert std.status is None and (host(st2.frames_seen) == 300).all()
    # update_weight = False: the weights stay, the masks differ
    fixed = run(dist, Y, state, alpha, update_weight=False)
    assert same(fixed[5], state[3]) and not same(fixed[0], a[0][:3])
    want = oc.recursive(Y, state, alpha, oc.EPS_AFF, update_weight=False)
    assert oc.relative(fixed[0], want[0], 'gamma') <= 16 * max(E_CASE[case, alpha][0], 1e-13)
    # affiliation_eps = 0: no clip
    free = run(dist, Y, state, alpha, eps=0.0)
    want = oc.recursive(Y, state, alpha, 0.0)
    assert oc.relative(free[0], want[0], 'gamma') <= 16 * max(E_CASE[case, alpha][0], 1e-13)
    assert np.abs(free[0].sum(axis=1) - 1).max() <= 8 * EPS


def test_first_frame_from_a_fitted_model(dist):
    """The first frame's gamma from the state of a device-fitted CACGMM is model.predict on that
    frame, within 1e-10 (the project's mask parity figure); affiliation_eps = 0, so no clip."""
    F, T, D, K = 5, 40, 4, 2
    rng = np.random.default_rng(7)
    y = (rng.standard_normal((F, T, D)) + 1j * rng.standard_normal((F, T, D))).astype(np.complex64)
    y[:, ::2] *= np.array([1.0, 0.2, 0.2, 0.2])
    np.random.seed(11)
    model = dist.CACGMMTrainer().fit(y, num_classes=K, iterations=5)
    want, qwant = model.predict(y[:, :1], return_quadratic_form=True)
    st = dist.OnlineCACGMMState.from_model(model)
    assert tuple(st.precision.shape) == (F, K, D, D) and tuple(st.weight.shape) == (F, K)
    assert np.abs(host(st.count) - 10.0 * host(st.weight)).max() <= 1e-14
    got, q = dist.recursive_cacgmm(y[:, :1], model, 0.99, affiliation_eps=0.0, layout='f t d',
                                   return_quadratic_form=True)
    assert got.shape == want.shape == (F, K, 1)
    print('first frame:', np.abs(got - want).max(), np.abs(q - qwant).max() / np.abs(qwant).max())
    assert np.abs(got - want).max() <= 1e-10
    assert np.abs(q - qwant).max() <= 1e-10 * np.abs(qwant).max()


def test_status(dist):
    from pb_bss_amd import _lib
    case, alpha = (3, 2, 65), 0.95
    Y, state = reference(case, alpha, 'complex128')[:2]
    clean = run(dist, Y, state, alpha)
    # a NaN sample in frame k of problem 1 of 3
    k = 40
    N = Y.copy()
    N[1, 2, k] = np.nan
    got = run(dist, N, state, alpha)
    assert host(got[6].status).tolist() == [0, _lib.ST_NONFINITE, 0]
    for i in (0, 1):
        assert same(got[i][1, :, :k], clean[i][1, :, :k]) and np.isnan(got[i][1, :, k:]).all()
    assert all(np.isnan(got[i][1]).all() for i in range(2, 6))
    assert all(same(got[i][[0, 2]], clean[i][[0, 2]]) for i in range(6))
    # an inf sample: nu = inf, z = NaN
    N = Y.copy()
    N[0, 0, 3] = np.inf
    got = run(dist, N, state, alpha)
    assert host(got[6].status).tolist() == [_lib.ST_NONFINITE, 0, 0]
    assert same(got[0][0, :, :3], clean[0][0, :, :3]) and np.isnan(got[0][0, :, 3:]).all()
    # an indefinite precision: flagged at frame 0
    Pbad = np.array(state[0])
    Pbad[2, 1] = -Pbad[2, 1]
    got = run(dist, Y, (Pbad,) + tuple(state[1:]), alpha)
    assert host(got[6].status).tolist() == [0, 0, _lib.ST_NONFINITE]
    assert np.isnan(got[0][2]).all() and np.isnan(got[1][2]).all()
    assert all(np.isnan(got[i][2]).all() for i in range(2, 6))
    assert all(same(got[i][:2], clean[i][:2]) for i in range(6))
    o_state = got[6]
    # a flagged state stays flagged
    g2, st2 = dist.recursive_cacgmm(Y[:, :, :4], None, alpha, state=o_state, return_state=True)
    assert host(st2.status).tolist() == [0, 0, _lib.ST_NONFINITE] and np.isnan(g2[2]).all()
    # the zero frame: the prior, q = 0
    z = oc.zero_frame(case)
    before = run(dist, Y[:, :, :z], state, alpha)
    assert same(clean[0][:, :, z], before[5]) and (clean[1][:, :, z] == 0).all()
    # only zeros: the state is the initial one but for frames_seen
    zeros = run(dist, np.zeros((oc.BATCH, 3, 5), np.complex64), state, alpha)
    assert (zeros[1] == 0).all() and same(zeros[0], np.repeat(state[3][:, :, None], 5, axis=2))
    assert all(same(zeros[i + 2], np.array(state[i])) for i in (1, 2, 3))
    assert same(np.tril(zeros[2], -1), np.tril(np.array(state[0]), -1))   # the triangle it reads
    assert same(np.diagonal(zeros[2], axis1=-2, axis2=-1).real,
                np.diagonal(state[0], axis1=-2, axis2=-1).real)
    assert (host(zeros[6].frames_seen) == 5).all() and (host(zeros[6].status) == 0).all()


def test_chain_wpe_cacgmm_mvdr(dist):
    """OnlineWPE.step_block -> OnlineCACGMM.step_block -> OnlineMVDR.step_block on device tensors,
    no transpose and no copy in between, against the three functional calls."""
    from pb_bss_amd import _lib, extraction, transform
    from pb_bss_amd.distribution import CACGMM, ComplexAngularCentralGaussian
    t = _lib.torch()
    F, D, K, Tb, alpha = 9, 4, 2, 20, 0.95
    rng = np.random.default_rng(3)
    Y = (rng.standard_normal((F, 3 * Tb, D)) + 1j * rng.standard_normal((F, 3 * Tb, D)))
    Y[:, :, 1:] *= 0.5
    Y = Y.astype(np.complex64)
    A = rng.standard_normal((F, K, D, D)) + 1j * rng.standard_normal((F, K, D, D))
    lam, vec = np.linalg.eigh(A @ A.conj().swapaxes(-1, -2) + np.eye(D))
    model = CACGMM(weight=np.full((F, K, 1), 0.5), cacg=ComplexAngularCentralGaussian(vec, lam))
    wpe = transform.OnlineWPE(taps=3, delay=2, alpha=0.999, channel=D, frequency_bins=F)
    gmm = dist.OnlineCACGMM(model, alpha)
    mvdr = extraction.OnlineMVDR(D, F, alpha, 0, 0.1)
    Yd = t.from_numpy(Y).cuda()
    blocks = [Yd[:, i * Tb:(i + 1) * Tb].contiguous() for i in range(3)]
    outs, affs = [], []
    for block in blocks:
        dry = wpe.step_block(block)
        t.cuda.synchronize()
        t.cuda.set_sync_debug_mode('error')
        try:
            aff = gmm.step_block(dry)
        finally:
            t.cuda.set_sync_debug_mode('default')
        outs.append(mvdr.step_block(dry, aff[:, 0], aff[:, 1]))
        affs.append(aff)
    assert dry.shape == (F, Tb, D) and aff.shape == (F, K, Tb) and outs[0].shape == (F, Tb)
    assert aff.dtype == t.float64 and outs[0].dtype == t.complex64
    dry_f = transform.recursive_wpe(Y, taps=3, delay=2, alpha=0.999, layout='f t d')
    aff_f = dist.recursive_cacgmm(dry_f, model, alpha, layout='f t d')
    x_f = extraction.recursive_mvdr_souden(dry_f, aff_f[:, 0], aff_f[:, 1], alpha, 0, 0.1,
                                           layout='f t d')
    assert np.isfinite(x_f).all() and np.isfinite(aff_f).all()
    assert same(host(t.cat(affs, dim=2)), aff_f) and same(host(t.cat(outs, dim=1)), x_f)
    assert (host(gmm.status) == 0).all() and (host(mvdr.status) == 0).all()


def test_t_zero_and_refusals(dist):
    case, alpha = (3, 2, 65), 0.95
    Y, state = reference(case, alpha, 'complex128')[:2]
    st = device_state(dist, state)
    G0, Q0, st0 = dist.recursive_cacgmm(Y[:, :, :0], None, alpha, state=st, return_state=True,
                                        return_quadratic_form=True)
    assert G0.shape == Q0.shape == (oc.BATCH, 2, 0) and G0.dtype == np.float64
    assert same(host(st0.precision), host(st.precision)) and (host(st0.frames_seen) == 0).all()
    assert same(host(st0.weight), host(st.weight)) and st0.status is None and st0 is not st
    G0 = dist.recursive_cacgmm(np.zeros((oc.BATCH, 0, 3), np.complex64), None, alpha, state=st,
                               layout='f t d')
    assert G0.shape == (oc.BATCH, 2, 0)
    with pytest.raises(NotImplementedError, match='ONLINE_CACGMM_MAX_D = 16'):
        dist.recursive_cacgmm(np.zeros((1, 17, 5), np.complex64), None, state=st)
    with pytest.raises(AssertionError):
        dist.recursive_cacgmm(Y[:, :2], None, alpha, state=st)      # D of the state is 3
    with pytest.raises(AssertionError):
        dist.recursive_cacgmm(Y.real.copy(), None, alpha, state=st)


def test_raw_c_abi_refuses_bad_arguments(dist):
    from pb_bss_amd import _lib
    t = _lib.torch()
    lib, h = _lib.load(), _lib.handle(0)
    B, D, K, T = 2, 4, 3, 40
    f64 = dict(dtype=t.float64, device='cuda')
    y = t.ones((B, 17, T), dtype=t.complex128, device='cuda')
    P = t.full((B, 9, 17, 17), 7.0, dtype=t.complex128, device='cuda')
    L, Lam, pi = (t.full((B, 9), 7.0, **f64) for _ in range(3))
    G, Q = (t.full((B, 9, T), 7.0, **f64) for _ in range(2))
    seen = t.full((B,), 7, dtype=t.int64, device='cuda')
    st = t.full((B,), 7, dtype=t.int32, device='cuda')
    p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED

    def call(y_=y, B_=B, D_=D, K_=K, T_=T, alpha=0.99, eps=1e-10, P_=P, L_=L, Lam_=Lam, pi_=pi,
             seen_=seen, G_=G, Q_=Q, st_=st, h_=h):
        return lib.pbbss_online_cacgmm(h_, p(y_), 1, B_, D_, K_, T_, D_ * T_, T_, 1, alpha, eps, 1,
                                       p(P_), p(L_), p(Lam_), p(pi_), p(seen_), p(G_), p(Q_),
                                       p(st_), None)
    for name in ('y_', 'P_', 'L_', 'Lam_', 'pi_', 'seen_', 'G_', 'st_', 'h_'):
        assert call(**{name: None}) == INV, name
    for name in ('B_', 'D_', 'K_', 'T_'):
        assert call(**{name: 0}) == INV, name
    assert call(K_=1) == INV and call(D_=1) == INV
    for alpha in (0.0, -0.5, 1.0 + 2.0 ** -52, float('nan'), float('inf')):
        assert call(alpha=alpha) == INV, alpha
    for eps in (-1e-10, 0.5, float('nan')):
        assert call(eps=eps) == INV, eps
    assert call(D_=17) == UNS and call(K_=9) == UNS and call(D_=17, K_=9) == UNS
    assert call(D_=17, K_=1) == INV
    t.cuda.synchronize()
    for a in (P, L, Lam, pi, G, Q):
        assert bool((a == 7.0).all())
    assert bool((st == 7).all()) and bool((seen == 7).all())
    # a valid call: out_quadratic_form may be null
    y4 = t.randn((B, D, T), dtype=t.complex128, device='cuda')
    P4 = t.eye(D, dtype=t.complex128, device='cuda').expand(B, K, D, D).contiguous()
    L4, Lam4, pi4 = t.zeros((B, K), **f64), t.ones((B, K), **f64), t.full((B, K), 1 / 3, **f64)
    G4 = t.full((B, K, T), 7.0, **f64)
    seen.zero_()
    assert call(y_=y4, P_=P4, L_=L4, Lam_=Lam4, pi_=pi4, G_=G4, Q_=None) == _lib.OK
    t.cuda.synchronize()
    assert bool((seen == T).all()) and bool((st == 0).all()) and bool((Q == 7.0).all())
    assert bool(t.isfinite(G4).all()) and bool(((G4 > 0) & (G4 < 1)).all())
    assert float((G4[:, :, 0] - 1 / 3).abs().max()) < 1e-15     # equal classes at the first frame
