"""GPU: frame-recursive WPE (csrc/wpe_online.hip; pb_bss_amd.transform.recursive_wpe, OnlineWPE,
online_wpe_step) against the NumPy restatement tests/oracle_wpe_online.py.

E_CASE is the restatement's own error (float64 run against the longdouble run, relative to
max |X|, max |G| and max |P|) for exactly the inputs of the sweep, the largest over both input
dtypes and over the causal and the given power; tests/test_wpe_online_oracle.py re-measures it and
keeps this copy within a factor of 4.  The device bound of a case is 16 * max(e_case, 1e-13)
relative to the maximum of the quantity, with the constants and the reasoning of
tests/test_gpu_wpe.py: the floor is about T eps for the longest row, 16 leaves room for another
summation order (the device adds its dot products on xor trees and multiplies by 1 / den where
NumPy's matmul adds in its own order).  complex64 output adds half an ulp of complex64 of max |X|
per component and is compared with the restatement rounded the same way.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle_wpe_online as oo

pytestmark = pytest.mark.gpu

E_CASE = {
    ((1, 1, 1, 8), 1.0): (6.5e-17, 4.4e-16, 2.2e-16),
    ((1, 1, 1, 8), 0.9999): (1.2e-16, 5.0e-16, 3.5e-16),
    ((1, 1, 1, 8), 0.99): (8.9e-17, 5.4e-16, 2.5e-16),
    ((2, 3, 1, 64), 1.0): (4.7e-16, 6.5e-16, 7.5e-16),
    ((2, 3, 1, 64), 0.9999): (8.6e-16, 4.9e-15, 1.8e-15),
    ((2, 3, 1, 64), 0.99): (7.0e-16, 3.5e-15, 1.6e-15),
    ((3, 3, 2, 65), 1.0): (7.6e-16, 4.1e-16, 1.3e-15),
    ((3, 3, 2, 65), 0.9999): (8.5e-16, 4.6e-15, 2.7e-15),
    ((3, 3, 2, 65), 0.99): (6.8e-16, 3.8e-15, 1.9e-15),
    ((4, 5, 3, 130), 1.0): (3.4e-15, 1.1e-15, 6.3e-15),
    ((4, 5, 3, 130), 0.9999): (7.2e-15, 9.2e-15, 6.6e-15),
    ((4, 5, 3, 130), 0.99): (1.1e-14, 7.1e-15, 1.3e-14),
    ((6, 10, 3, 300), 1.0): (1.7e-14, 2.2e-15, 3.6e-14),
    ((6, 10, 3, 300), 0.9999): (2.0e-14, 2.1e-14, 5.3e-14),
    ((6, 10, 3, 300), 0.99): (5.5e-14, 2.5e-14, 1.3e-13),
    ((8, 10, 3, 300), 1.0): (1.4e-14, 5.4e-15, 4.4e-14),
    ((8, 10, 3, 300), 0.9999): (2.1e-14, 2.2e-14, 9.5e-14),
    ((8, 10, 3, 300), 0.99): (6.7e-14, 5.1e-14, 2.8e-13),
    ((16, 6, 3, 200), 1.0): (1.2e-14, 2.5e-15, 2.7e-14),
    ((16, 6, 3, 200), 0.9999): (1.5e-14, 1.5e-14, 4.5e-14),
    ((16, 6, 3, 200), 0.99): (2.6e-14, 1.8e-14, 7.7e-14),
    ((8, 12, 3, 257), 1.0): (1.9e-14, 2.9e-15, 4.5e-14),
    ((8, 12, 3, 257), 0.9999): (2.8e-14, 2.1e-14, 5.1e-14),
    ((8, 12, 3, 257), 0.99): (5.3e-14, 2.5e-14, 1.1e-13),
    ((2, 3, 1, 1000), 1.0): (9.3e-16, 5.1e-16, 1.6e-15),
    ((2, 3, 1, 1000), 0.9999): (1.2e-15, 4.1e-14, 1.8e-14),
    ((2, 3, 1, 1000), 0.99): (1.7e-15, 6.5e-15, 6.4e-15),
    ((2, 3, 1, 31), 1.0): (4.0e-16, 2.7e-16, 9.9e-16),
    ((2, 3, 1, 31), 0.9999): (5.1e-16, 2.2e-15, 1.2e-15),
    ((2, 3, 1, 31), 0.99): (5.3e-16, 1.7e-15, 1.1e-15),
    ((2, 3, 1, 32), 1.0): (4.9e-16, 3.3e-16, 1.2e-15),
    ((2, 3, 1, 32), 0.9999): (4.8e-16, 2.6e-15, 1.1e-15),
    ((2, 3, 1, 32), 0.99): (3.6e-16, 2.4e-15, 1.1e-15),
    ((2, 3, 1, 33), 1.0): (3.3e-16, 5.6e-16, 2.6e-16),
    ((2, 3, 1, 33), 0.9999): (4.5e-16, 2.3e-15, 2.9e-16),
    ((2, 3, 1, 33), 0.99): (4.7e-16, 1.3e-15, 3.5e-16),
    ((4, 8, 2, 70), 1.0): (3.4e-15, 8.3e-16, 6.0e-15),
    ((4, 8, 2, 70), 0.9999): (4.1e-15, 5.5e-15, 6.7e-15),
    ((4, 8, 2, 70), 0.99): (4.4e-15, 5.0e-15, 7.8e-15),
    ((3, 11, 2, 70), 1.0): (2.0e-15, 7.5e-16, 4.5e-15),
    ((3, 11, 2, 70), 0.9999): (2.3e-15, 5.4e-15, 5.2e-15),
    ((3, 11, 2, 70), 0.99): (5.0e-15, 5.1e-15, 1.4e-14),
}
EPS = 2.0 ** -52


@pytest.fixture(scope='module')
def tw():
    from pb_bss_amd import _lib
    from pb_bss_amd import transform
    _lib.require_gpu()
    return transform


@functools.lru_cache(maxsize=None)
def reference(case, alpha, dtype_name, given):
    """(Y (BATCH, D, T), power (BATCH, T) or None, X, inv_cov, filter_taps) of the restatement."""
    D, taps, delay, T = case
    Y = oo.case_input(case, np.dtype(dtype_name))
    pw = oo.case_power(case, np.dtype(dtype_name)) if given else None
    X, P, G, flagged = oo.recursive(Y, taps, delay, alpha, pw)
    assert not flagged.any()
    for a in (Y, pw, X, P, G):
        if a is not None:
            a.setflags(write=False)
    return Y, pw, X, P, G


def distance(got, want):
    """(error, half an ulp of the output type), both relative to max |want|."""
    scale = np.abs(want).max()
    if got.dtype == np.complex64:
        w = want.astype(np.complex64)
        err = max(np.abs(got.real.astype(np.float64) - w.real).max(),
                  np.abs(got.imag.astype(np.float64) - w.imag).max())
        return err / scale, 2.0 ** -24
    return np.abs(got - want).max() / scale, 0.0


def host(a):
    return a.detach().cpu().numpy()


def run(tw, Y, taps, delay, alpha, pw=None, **kw):
    """recursive_wpe on NumPy input -> (X, inv_cov, filter_taps, state)."""
    X, st = tw.recursive_wpe(Y, taps, delay, alpha, pw, return_state=True, **kw)
    return X, host(st.inv_cov), host(st.filter_taps), st


@pytest.mark.parametrize('alpha', oo.ALPHAS)
@pytest.mark.parametrize('case', oo.CASES, ids=str)
def test_parity(tw, case, alpha):
    D, taps, delay, T = case
    M = D * taps
    worst = 0.0
    for dtype_name in ('complex128', 'complex64'):
        for given in (False, True):
            Y, pw, Xw, Pw, Gw = reference(case, alpha, dtype_name, given)
            for B in (1, oo.BATCH):
                X, P, G, st = run(tw, Y[:B], taps, delay, alpha, None if pw is None else pw[:B])
                assert X.dtype == Y.dtype and X.shape == Y[:B].shape
                assert P.shape == (B, M, M) and G.shape == (B, M, D)
                assert P.dtype == G.dtype == np.complex128
                assert (host(st.frames_seen) == T).all()
                assert (P == P.conj().swapaxes(-1, -2)).all()       # Hermitian to the bit
                assert (np.diagonal(P, axis1=-2, axis2=-1).imag == 0).all()
                for name, got, want, e in (('X', X, Xw[:B], E_CASE[case, alpha][0]),
                                           ('G', G, Gw[:B], E_CASE[case, alpha][1]),
                                           ('P', P, Pw[:B], E_CASE[case, alpha][2])):
                    err, ulp = distance(got, want)
                    bound = 16 * max(e, 1e-13) + ulp
                    print(f'{case} a={alpha} {dtype_name} given={given} B={B} {name}: {err:.2e} '
                          f'(bound {bound:.2e})')
                    worst = max(worst, (err - ulp) / (16 * max(e, 1e-13)))
                    assert err <= bound, (case, alpha, dtype_name, given, B, name, err, bound)
    print(f'{case} a={alpha}: worst {worst:.3f} of the bound')


@pytest.mark.parametrize('alpha', oo.ALPHAS)
@pytest.mark.parametrize('case', [(2, 3, 1, 64), (4, 8, 2, 70), (6, 10, 3, 300), (8, 12, 3, 257),
                                  (2, 3, 1, 1000)], ids=str)
def test_filter_is_the_batch_solution_of_the_devices_own_correlations(tw, case, alpha):
    D, taps, delay, T = case
    for given in (False, True):
        Y, pw, _, _, _ = reference(case, alpha, 'complex128', given)
        lam = pw if given else np.stack([oo.causal_power(y, taps, delay) for y in Y])
        _, _, G, _ = run(tw, Y, taps, delay, alpha, pw)
        w = alpha ** np.arange(T - 1, -1, -1.0) / lam
        R, C = tw.get_correlations(Y, w, taps, delay)
        for b in range(oo.BATCH):
            A = alpha ** T * np.eye(D * taps) + R[b]
            Gw, cond = np.linalg.solve(A, C[b]), np.linalg.cond(A)
            err, tol = np.abs(G[b] - Gw).max(), 16 * cond * EPS * np.abs(Gw).max()
            print(f'{case} a={alpha} given={given} b={b}: {err:.2e} (tol {tol:.2e}, cond {cond:.1e})')
            assert err <= tol, (case, alpha, given, b, err, tol, cond)


def same(a, b):
    """equal bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('case', [(2, 3, 1, 130), (16, 6, 3, 100)], ids=str)
def test_blocking_is_bitwise_invisible(tw, case):
    from pb_bss_amd import _lib
    t = _lib.torch()
    D, taps, delay, T = case
    alpha = 0.99
    Y = oo.synth(oo.BATCH, D, T, seed=5).astype(np.complex64)
    pw = oo.causal_power(Y[0].astype(np.complex128), taps, delay)[None] * [[1.0], [2.0], [0.5]] + 0.1
    for power in (None, pw):
        X, P, G, _ = run(tw, Y, taps, delay, alpha, power)
        # blocks of lengths 1, 1, 7, 64, rest, each continuing from the returned state
        st, outs, t0 = None, [], 0
        for n in (1, 1, 7, 64, T - 73):
            x, st = tw.recursive_wpe(Y[:, :, t0:t0 + n], taps, delay, alpha,
                                     None if power is None else power[:, t0:t0 + n],
                                     state=st, return_state=True)
            outs.append(x)
            t0 += n
        assert same(np.concatenate(outs, axis=-1), X)
        assert same(host(st.inv_cov), P) and same(host(st.filter_taps), G)
        assert (host(st.frames_seen) == T).all()
        want_hist = Y[:, :, T - taps - delay:].astype(np.complex128)
        assert same(host(st.history), want_hist)
    # OnlineWPE frame by frame and in blocks (the causal power)
    X, P, G, _ = run(tw, Y, taps, delay, alpha)
    by_frame = tw.OnlineWPE(taps, delay, alpha, channel=D, frequency_bins=oo.BATCH)
    frames = [by_frame.step_frame(Y[:, :, i]) for i in range(T)]
    assert frames[0].shape == (oo.BATCH, D) and isinstance(frames[0], np.ndarray)
    assert same(np.stack(frames, axis=-1), X)
    assert same(host(by_frame.inv_cov), P) and same(host(by_frame.filter_taps), G)
    assert by_frame.buffer.shape == (taps + delay, oo.BATCH, D)
    assert same(host(by_frame.buffer), np.moveaxis(want_hist, -1, 0))
    by_block = tw.OnlineWPE(taps, delay, alpha, channel=D, frequency_bins=oo.BATCH)
    Yd = t.from_numpy(np.ascontiguousarray(Y.swapaxes(1, 2))).cuda()       # (F, T, D)
    blocks = [by_block.step_block(Yd[:, a:b]) for a, b in ((0, 33), (33, 34), (34, T))]
    assert all(x.is_cuda for x in blocks)
    assert same(host(t.cat(blocks, dim=1)), np.ascontiguousarray(X.swapaxes(1, 2)))
    assert same(host(by_block.inv_cov), P)
    # a fixed power estimate per bin
    fixed = np.array([0.5, 1.0, 2.0])
    Xf, Pf, _, _ = run(tw, Y, taps, delay, alpha, np.repeat(fixed[:, None], T, axis=1))
    with_fixed = tw.OnlineWPE(taps, delay, alpha, channel=D, frequency_bins=oo.BATCH,
                              power_estimate=fixed)
    assert same(host(with_fixed.step_block(Yd)), np.ascontiguousarray(Xf.swapaxes(1, 2)))
    assert same(host(with_fixed.inv_cov), Pf)
    # online_wpe_step fed by hand, with the given power
    X, P, G, _ = run(tw, Y, taps, delay, alpha, pw)
    M, H = D * taps, taps + delay
    buf = np.zeros((H + 1, oo.BATCH, D), np.complex64)
    Ph = np.broadcast_to(np.eye(M, dtype=np.complex128), (oo.BATCH, M, M)).copy()
    Gh = np.zeros((oo.BATCH, M, D), np.complex128)
    for i in range(T):
        buf = np.concatenate([buf[1:], Y[None, :, :, i]])
        pred, Ph, Gh = tw.online_wpe_step(buf, pw[:, i], Ph, Gh, alpha, taps, delay)
        assert same(pred, X[:, :, i]), i
    assert same(Ph, P) and same(Gh, G)
    # tensors in, tensors out, inputs untouched
    bd, Pd, Gd = (t.from_numpy(a).cuda() for a in (buf, P, G))
    copies = [a.clone() for a in (bd, Pd, Gd)]
    pred, P2, G2 = tw.online_wpe_step(bd, t.from_numpy(pw[:, -1]).cuda(), Pd, Gd, alpha, taps, delay)
    assert pred.is_cuda and P2.is_cuda and G2.is_cuda and pred.dtype == t.complex64
    assert all(bool((a == b).all()) for a, b in zip(copies, (bd, Pd, Gd)))
    assert P2.data_ptr() != Pd.data_ptr() and G2.data_ptr() != Gd.data_ptr()


def test_determinism_and_batch_independence(tw):
    case = (6, 10, 3, 300)
    Y, _, _, _, _ = reference(case, 0.9999, 'complex64', False)
    Y5 = np.concatenate([Y, Y[:2] * 0.5 + Y[1:] * 0.25])
    a = run(tw, Y5, 10, 3, 0.9999)
    again = run(tw, Y5, 10, 3, 0.9999)
    assert all(same(a[i], again[i]) for i in range(3))
    for b in range(5):
        one = run(tw, Y5[b], 10, 3, 0.9999)
        assert same(a[0][b], one[0]) and same(a[1][b], one[1][0]) and same(a[2][b], one[2][0]), b


def test_layout_and_chain_into_the_mixture_model(tw):
    from pb_bss_amd import _lib
    from pb_bss_amd.distribution import CACGMMTrainer
    t = _lib.torch()
    Y, _, _, _, _ = reference((4, 5, 3, 130), 0.99, 'complex64', False)
    a = tw.recursive_wpe(np.ascontiguousarray(Y.swapaxes(-1, -2)), 5, 3, 0.99, layout='f t d')
    b = tw.recursive_wpe(Y, 5, 3, 0.99)
    assert a.shape == (oo.BATCH, 130, 4) and same(a, np.ascontiguousarray(b.swapaxes(-1, -2)))
    with pytest.raises(ValueError):
        tw.recursive_wpe(Y, 5, 3, 0.99, layout='t f d')
    # audio -> stft(layout='f t d') -> recursive_wpe(layout='f t d') -> fit, all on the device
    rng = np.random.default_rng(3)
    audio = t.from_numpy(rng.standard_normal((4, 4096))).cuda()
    S = tw.stft(audio, size=128, shift=32, layout='f t d')
    F, T, D = S.shape
    assert D == 4 and S.is_cuda
    X = tw.recursive_wpe(S, 3, 2, 0.999, layout='f t d')
    assert X.is_cuda and X.is_contiguous() and X.shape == S.shape and X.dtype == S.dtype
    Xt = tw.recursive_wpe(S.transpose(1, 2).contiguous(), 3, 2, 0.999).transpose(1, 2).contiguous()
    assert bool((X == Xt).all())
    init = rng.uniform(size=(F, 2, T))
    init /= init.sum(axis=1, keepdims=True)
    masks = [CACGMMTrainer().fit(x, initialization=init, iterations=3).predict(x)
             for x in (X, Xt)]
    m0, m1 = (_lib.to_host(m) if _lib.is_torch(m) else m for m in masks)
    assert np.isfinite(m0).all() and (m0 == m1).all()


def test_edges(tw):
    from pb_bss_amd import _lib
    case, alpha = (2, 3, 1, 64), 0.99
    Y, _, Xw, _, _ = reference(case, alpha, 'complex128', False)
    X, P, G, _ = run(tw, Y, 3, 1, alpha)
    # an all-zero problem inside a batch: zeros, gain 0, P only divided by alpha
    Z = Y.copy()
    Z[1] = 0
    Xz, Pz, Gz, st = run(tw, Z, 3, 1, alpha)
    assert (Xz[1] == 0).all() and (Gz[1] == 0).all()
    assert same(Xz[[0, 2]], X[[0, 2]]) and same(Pz[[0, 2]], P[[0, 2]]) and same(Gz[[0, 2]], G[[0, 2]])
    ref = oo.recursive(Z, 3, 1, alpha)
    assert np.abs(Pz[1] - ref[1][1]).max() <= 64 * EPS * np.abs(ref[1][1]).max()
    # an all-zero stretch inside a live stream: gain 0 there, finite output, against the restatement
    S = Y.copy()
    S[:, :, 20:40] = 0
    Xs, Ps, Gs, _ = run(tw, S, 3, 1, alpha)
    ref = oo.recursive(S, 3, 1, alpha)
    assert np.isfinite(Xs).all() and (Xs[:, :, 24:40] == 0).all()   # the past is zero from 24 on
    mid = run(tw, S[:, :, :25], 3, 1, alpha)
    later = run(tw, S[:, :, :39], 3, 1, alpha)
    assert same(mid[2], later[2])                     # G does not move over frames of zeros
    for got, want in zip((Xs, Ps, Gs), ref):
        assert np.abs(got - want).max() <= 16 * 1e-13 * np.abs(want).max()
    # delay = 0 against the restatement; fewer frames than taps + delay
    for delay, T in ((0, 64), (1, 3), (2, 1), (3, 5)):
        got = run(tw, Y[:, :, :T], 3, delay, alpha)
        want = oo.recursive(Y[:, :, :T], 3, delay, alpha)
        for g, w in zip(got[:3], want):
            assert np.abs(g - w).max() <= 16 * 1e-13 * np.abs(w).max(), (delay, T)
        assert (host(got[3].frames_seen) == T).all()
        assert same(host(got[3].history)[:, :, 3 + delay - min(T, 3 + delay):],
                    Y[:, :, max(0, T - 3 - delay):T])
    # a NaN frame sets the status word of its problem only; its output is NaN from there on
    N = Y.copy()
    N[1, 0, 30] = np.nan
    y = _lib.to_device(N)
    state = tw.OnlineWPEState.initial(oo.BATCH, 2, 3, 1)
    from pb_bss_amd import engine
    x, status = engine.wpe_online(y, 3, 1, alpha, None, state.inv_cov, state.filter_taps,
                                  state.history, state.frames_seen)
    assert host(status).tolist() == [0, _lib.ST_NONFINITE, 0]
    x = host(x)
    assert same(x[[0, 2]], X[[0, 2]]) and same(x[1, :, :30], X[1, :, :30])
    assert np.isnan(x[1, :, 30:]).all()
    assert np.isnan(host(state.inv_cov)[1]).all() and np.isnan(host(state.filter_taps)[1]).all()
    assert same(host(state.inv_cov)[[0, 2]], P[[0, 2]])
    ref = oo.recursive(N, 3, 1, alpha)
    assert ref[3].tolist() == [False, True, False] and np.isnan(ref[0][1, :, 30:]).all()
    # the status words through the public interface
    _, stn = tw.recursive_wpe(N, 3, 1, alpha, return_state=True)
    assert host(stn.status).tolist() == [0, _lib.ST_NONFINITE, 0]
    assert host(st.status).tolist() == [0, 0, 0]
    o = tw.OnlineWPE(3, 1, alpha, channel=2, frequency_bins=oo.BATCH)
    assert o.status is None
    o.step_block(np.ascontiguousarray(N.swapaxes(1, 2)))
    assert host(o.status).tolist() == [0, _lib.ST_NONFINITE, 0]
    # T = 0: empty output, the state unchanged
    X0, st0 = tw.recursive_wpe(Y[:, :, :0], 3, 1, alpha, state=st, return_state=True)
    assert X0.shape == (oo.BATCH, 2, 0) and same(host(st0.inv_cov), host(st.inv_cov))
    assert (host(st0.frames_seen) == 64).all()
    X0, st0 = tw.recursive_wpe(Y[:, :, :0], 3, 1, alpha, return_state=True)
    assert (host(st0.inv_cov) == np.eye(6)).all() and (host(st0.frames_seen) == 0).all()
    o = tw.OnlineWPE(3, 1, alpha, channel=2, frequency_bins=oo.BATCH)
    assert o.step_block(np.zeros((oo.BATCH, 0, 2), np.complex64)).shape == (oo.BATCH, 0, 2)
    with pytest.raises(AssertionError):
        tw.recursive_wpe(Y.real.copy(), 3, 1)
    with pytest.raises(AssertionError):
        tw.recursive_wpe(Y, 3, 1, alpha=1.5)
    with pytest.raises(NotImplementedError, match='WPE_MAX_M = 96'):
        tw.recursive_wpe(np.zeros((8, 50), np.complex64), taps=13)
    with pytest.raises(NotImplementedError, match='WPE_MAX_D = 16'):
        tw.recursive_wpe(np.zeros((17, 50), np.complex64), taps=1)
    with pytest.raises(NotImplementedError, match='WPE_ONLINE_MAX_RING = 2048'):
        tw.recursive_wpe(np.zeros((16, 50), np.complex64), taps=2, delay=127)
    with pytest.raises(NotImplementedError, match='WPE_MAX_M = 96'):
        tw.OnlineWPE(taps=13, channel=8, frequency_bins=4)


def test_kinds_and_dtypes(tw):
    from pb_bss_amd import _lib
    t = _lib.torch()
    Y, _, _, _, _ = reference((3, 3, 2, 65), 0.99, 'complex64', False)
    one = tw.recursive_wpe(Y[0], 3, 2, 0.99)
    for y in (Y, Y.astype(np.complex128), Y[0], Y.reshape(3, 1, 3, 65)):
        x = tw.recursive_wpe(y, 3, 2, 0.99)
        assert isinstance(x, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape
        if y.dtype == np.complex64:
            assert same(x.reshape(-1, 3, 65)[0], one)
    yd = t.from_numpy(Y.copy()).cuda()
    xd, st = tw.recursive_wpe(yd, 3, 2, 0.99, return_state=True)
    assert xd.is_cuda and xd.dtype == t.complex64
    assert same(host(xd), tw.recursive_wpe(Y, 3, 2, 0.99))
    assert all(a.is_cuda for a in (st.inv_cov, st.filter_taps, st.history, st.frames_seen))
    assert st.inv_cov.dtype == st.filter_taps.dtype == st.history.dtype == t.complex128
    assert st.frames_seen.dtype == t.int64
    # the state passed in is not modified
    keep = st.clone()
    tw.recursive_wpe(yd, 3, 2, 0.99, state=st)
    assert bool((keep.inv_cov == st.inv_cov).all()) and bool((keep.frames_seen == st.frames_seen).all())
    pw = t.from_numpy(oo.case_power((3, 3, 2, 65), np.complex64)).cuda()
    assert same(host(tw.recursive_wpe(yd, 3, 2, 0.99, pw)),
                tw.recursive_wpe(Y, 3, 2, 0.99, host(pw)))


def test_raw_c_abi_refuses_bad_arguments(tw):
    from pb_bss_amd import _lib
    t = _lib.torch()
    lib, h = _lib.load(), _lib.handle(0)
    B, D, T, taps, delay = 2, 4, 40, 3, 2
    M, H = D * taps, taps + delay
    c128 = dict(dtype=t.complex128, device='cuda')
    y = t.ones((B, D, T), **c128)
    x = t.full((B, D, T), 7.0, **c128)
    P = t.full((B, M, M), 7.0, **c128)
    G = t.full((B, M, D), 7.0, **c128)
    hist = t.full((B, D, H), 7.0, **c128)
    big = t.full((16 * 129,), 7.0, **c128)
    seen = t.full((B,), 7, dtype=t.int64, device='cuda')
    st = t.full((B,), 7, dtype=t.int32, device='cuda')
    pw = t.ones((B, T), dtype=t.float64, device='cuda')
    p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED

    def call(y_=y, B_=B, D_=D, T_=T, taps_=taps, delay_=delay, alpha=0.99, pw_=pw, P_=P, G_=G,
             hist_=hist, seen_=seen, x_=x, st_=st):
        return lib.pbbss_wpe_online(h, p(y_), 1, B_, D_, T_, D_ * T_, T_, 1, taps_, delay_, alpha,
                                    p(pw_), p(P_), p(G_), p(hist_), p(seen_), p(x_), p(st_), None)
    for name in ('y_', 'P_', 'G_', 'hist_', 'seen_', 'x_', 'st_'):
        assert call(**{name: None}) == INV, name
    for name in ('B_', 'D_', 'T_', 'taps_'):
        assert call(**{name: 0}) == INV, name
    assert call(delay_=-1) == INV
    for alpha in (0.0, -0.5, 1.0 + 2.0 ** -52, float('nan'), float('inf')):
        assert call(alpha=alpha) == INV, alpha
    assert call(taps_=25) == UNS                                    # M = 100
    assert call(D_=17, taps_=1, T_=1, B_=1) == UNS
    assert call(D_=17, taps_=0, T_=1, B_=1) == INV and call(D_=17, taps_=1, delay_=-1, T_=1, B_=1) == INV
    assert call(D_=16, taps_=1, delay_=128, T_=1, B_=1, hist_=big) == UNS  # D (taps + delay) = 2064
    t.cuda.synchronize()
    for a in (x, P, G, hist, big):
        assert bool((a == 7.0).all())
    assert bool((st == 7).all()) and bool((seen == 7).all())
