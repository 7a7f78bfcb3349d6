"""GPU: WPE dereverberation (csrc/wpe.hip, pb_bss_amd.transform.wpe) against the NumPy restatement
tests/oracle_wpe.py.

E_CASE is the restatement's own error (float64 run against the longdouble run, relative to
max |X|) after one and after three iterations, for exactly the inputs of the sweep, the largest
over both statistics modes and both input dtypes; tests/test_wpe_oracle.py re-measures it and
keeps this copy within a factor of 4.  The device bound of a case is 16 * max(e_case, 1e-13)
relative to max |X|: the floor is about T eps for the longest row, 16 leaves room for another
summation order and for Cholesky where the restatement factors by pivoted LU (each backward
stable, with an error of the same cond(R) eps kind as the restatement's own).  complex64 output
adds half an ulp of complex64 of max |X| per component and is compared with the restatement
rounded the same way.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle_wpe as ow

pytestmark = pytest.mark.gpu

E_CASE = {
    (1, 1, 1, 8): (7.8e-17, 1.8e-16),
    (1, 4, 1, 64): (8.1e-16, 1.6e-12),
    (2, 3, 1, 63): (1.6e-15, 7.7e-15),
    (2, 3, 1, 64): (2.3e-15, 2.4e-13),
    (2, 3, 1, 65): (9.6e-16, 5.0e-15),
    (3, 3, 2, 65): (4.4e-14, 1.7e-13),
    (4, 5, 3, 130): (1.0e-12, 1.2e-11),
    (5, 7, 2, 200): (1.1e-12, 4.9e-09),
    (6, 10, 3, 300): (2.3e-12, 2.0e-08),
    (8, 10, 3, 257): (4.5e-12, 3.2e-08),
    (8, 10, 3, 300): (3.7e-12, 1.3e-09),
    (8, 12, 3, 400): (6.2e-12, 1.6e-09),
    (16, 5, 3, 320): (5.1e-12, 5.6e-09),
    (2, 3, 1, 127): (1.9e-15, 3.7e-14),
    (2, 3, 1, 128): (5.6e-15, 4.9e-14),
    (2, 3, 1, 129): (1.9e-15, 1.7e-14),
    (2, 3, 1, 255): (1.5e-15, 2.7e-15),
    (2, 3, 1, 256): (8.7e-15, 1.8e-14),
    (4, 12, 2, 200): (2.4e-12, 3.4e-10),
    (9, 3, 1, 129): (3.3e-13, 6.9e-11),
}
EPS = 2.0 ** -52


@pytest.fixture(scope='module')
def tw():
    from pb_bss_amd import _lib
    from pb_bss_amd import transform
    _lib.require_gpu()
    return transform


@functools.lru_cache(maxsize=None)
def reference(case, dtype_name, mode):
    """(input (BATCH, D, T), [X after one iteration, after three]) of the restatement."""
    D, taps, delay, T = case
    Y = ow.case_input(case, np.dtype(dtype_name))
    snaps = ow.wpe(Y, taps, delay, 3, 0, mode, snapshots=True)
    for a in (Y, snaps[0], snaps[2]):
        a.setflags(write=False)
    return Y, {1: snaps[0], 3: snaps[2]}


def distance(got, want):
    """(error, half an ulp of the output type), both relative to max |want|."""
    scale = np.abs(want).max()
    if got.dtype == np.complex64:
        w = want.astype(np.complex64)
        err = max(np.abs(got.real.astype(np.float64) - w.real).max(),
                  np.abs(got.imag.astype(np.float64) - w.imag).max())
        return err / scale, 2.0 ** -24
    return np.abs(got - want).max() / scale, 0.0


def check_sweep(tw, case, iterations):
    D, taps, delay, T = case
    e = E_CASE[case][0 if iterations == 1 else 1]
    worst = 0.0
    for dtype_name in ('complex128', 'complex64'):
        for mode in ('full', 'valid'):
            Y, want = reference(case, dtype_name, mode)
            for B in (1, ow.BATCH):
                X = tw.wpe(Y[:B], taps, delay, iterations, statistics_mode=mode)
                assert X.dtype == Y.dtype and X.shape == Y[:B].shape
                err, ulp = distance(X, want[iterations][:B])
                bound = 16 * max(e, 1e-13) + ulp
                print(f'{case} it={iterations} {dtype_name} {mode} B={B}: {err:.2e} '
                      f'(bound {bound:.2e})')
                worst = max(worst, (err - ulp) / (16 * max(e, 1e-13)))
                assert err <= bound, (case, iterations, dtype_name, mode, B, err, bound)
    print(f'{case} it={iterations}: worst {worst:.3f} of the bound')


@pytest.mark.parametrize('case', ow.CASES, ids=str)
def test_one_iteration_parity(tw, case):
    check_sweep(tw, case, 1)


@pytest.mark.parametrize('case', ow.CASES, ids=str)
def test_three_iteration_parity(tw, case):
    check_sweep(tw, case, 3)


@pytest.mark.parametrize('context', [0, 2, np.inf])
def test_power_inverse(tw, context):
    X = ow.synth(3, 3, 300, seed=9)
    X[1, :, 40:60] *= 1e-7          # a silent stretch that reaches the 1e-10 floor
    X[2] = 0                        # an all-zero problem: weight 0
    for dtype in (np.complex128, np.complex64):
        x = X.astype(dtype)
        p, inv = tw.get_power(x, context), tw.get_power_inverse(x, context)
        assert p.dtype == inv.dtype == np.float64 and p.shape == inv.shape == (3, 300)
        np.testing.assert_allclose(p, ow.power(x.astype(np.complex128), context), rtol=1e-13)
        want = ow.power_inverse(x.astype(np.complex128), context)
        np.testing.assert_allclose(inv, want, rtol=1e-13)
        assert (inv[2] == 0).all()
        if context == 0:
            assert (inv[1, 40:60] == inv[1].max()).all() and inv[1, 0] < inv[1].max()


@pytest.mark.parametrize('case', [(2, 3, 1, 64), (5, 7, 2, 200), (8, 12, 3, 400)], ids=str)
def test_parts_and_their_composition(tw, case):
    D, taps, delay, T = case
    M = D * taps
    for dtype_name in ('complex128', 'complex64'):
        for mode in ('full', 'valid'):
            Y, want = reference(case, dtype_name, mode)
            Y128 = Y.astype(np.complex128)
            inv = tw.get_power_inverse(Y)
            R, P = tw.get_correlations(Y, inv, taps, delay, mode)
            assert R.dtype == P.dtype == np.complex128
            assert R.shape == (ow.BATCH, M, M) and P.shape == (ow.BATCH, M, D)
            assert (R == R.conj().swapaxes(-1, -2)).all()            # Hermitian to the bit
            G = tw.get_filter_matrix(R, P)
            X = tw.perform_filter_operation(Y, G, taps, delay)
            assert G.dtype == np.complex128 and X.dtype == Y.dtype
            for b in range(ow.BATCH):
                Rw, Pw = ow.correlations(Y128[b], inv[b], taps, delay, mode)
                assert np.abs(R[b] - Rw).max() <= 16 * T * EPS * np.abs(Rw).max()
                assert np.abs(P[b] - Pw).max() <= 16 * T * EPS * np.abs(Pw).max()
                # G against LAPACK's solve of the device's own R, P: both backward stable, so
                # each is within about cond(R) eps of the exact solution
                Gw = np.linalg.solve(R[b], P[b])
                cond = np.linalg.cond(R[b])
                assert np.abs(G[b] - Gw).max() <= 16 * cond * EPS * np.abs(Gw).max(), cond
                # the filter with the device's own G: M + 1 rounded products and sums per entry
                Xw = ow.apply_filter(Y128[b], G[b], taps, delay)
                size = np.abs(Y128[b]).max() * (1 + np.abs(G[b]).sum(axis=0).max())
                err, ulp = distance(X[b], Xw)
                assert err * np.abs(Xw).max() <= 4 * (M + 2) * EPS * size + ulp * np.abs(Xw).max()
            err, ulp = distance(X, want[1])
            assert err <= 16 * max(E_CASE[case][0], 1e-13) + ulp, (case, dtype_name, mode, err)


def test_layout_and_chain_into_the_mixture_model(tw):
    from pb_bss_amd import _lib
    from pb_bss_amd.distribution import CACGMMTrainer
    t = _lib.torch()
    Y, _ = reference((4, 5, 3, 130), 'complex64', 'full')
    a = tw.wpe(np.ascontiguousarray(Y.swapaxes(-1, -2)), 5, 3, 2, layout='f t d')
    b = tw.wpe(Y, 5, 3, 2)
    assert a.shape == (ow.BATCH, 130, 4) and (a == b.swapaxes(-1, -2)).all()
    # audio -> stft(layout='f t d') -> wpe(layout='f t d') -> fit, all on the device
    rng = np.random.default_rng(3)
    audio = t.from_numpy(rng.standard_normal((4, 4096))).cuda()
    S = tw.stft(audio, size=128, shift=32, layout='f t d')
    F, T, D = S.shape
    assert D == 4 and S.is_cuda
    X = tw.wpe(S, 3, 2, 2, layout='f t d')
    assert X.is_cuda and X.is_contiguous() and X.shape == S.shape and X.dtype == S.dtype
    Xt = tw.wpe(S.transpose(1, 2).contiguous(), 3, 2, 2).transpose(1, 2).contiguous()
    assert bool((X == Xt).all())
    init = rng.uniform(size=(F, 2, T))
    init /= init.sum(axis=1, keepdims=True)
    masks = [CACGMMTrainer().fit(x, initialization=init, iterations=3).predict(x)
             for x in (X, Xt)]
    m0, m1 = (_lib.to_host(m) if _lib.is_torch(m) else m for m in masks)
    assert np.isfinite(m0).all() and (m0 == m1).all()


def test_determinism_and_batch_independence(tw):
    case = (6, 10, 3, 300)
    Y, _ = reference(case, 'complex64', 'full')
    Y5 = np.concatenate([Y, Y[:2] * 0.5 + Y[1:] * 0.25])
    a = tw.wpe(Y5, 10, 3, 3)
    assert (a == tw.wpe(Y5, 10, 3, 3)).all()
    for b in range(5):
        assert (a[b] == tw.wpe(Y5[b], 10, 3, 3)).all(), b


def test_edges(tw):
    from pb_bss_amd import _lib
    t = _lib.torch()
    Y, _ = reference((2, 3, 1, 64), 'complex128', 'full')
    x0 = tw.wpe(Y, 3, 1, 0)
    assert (x0 == Y).all() and not np.shares_memory(x0, Y)
    yt = t.from_numpy(Y.copy()).cuda()
    x0 = tw.wpe(yt, 3, 1, 0)
    assert bool((x0 == yt).all()) and x0.data_ptr() != yt.data_ptr()
    # exactly singular: R = 0 -> the status word -> lstsq on the host -> X = Y
    for T, delay in ((1, 1), (3, 3), (2, 5)):
        y = Y[:, :, :T].copy()
        assert (tw.wpe(y, 3, delay, 2) == y).all(), (T, delay)
        yd = t.from_numpy(y).cuda()
        assert bool(t.isnan(tw.wpe(yd, 3, delay, 2).real).all())   # unchecked: NaN on the device
        assert bool((tw.wpe(yd, 3, delay, 2, check=True) == yd).all())
    # an all-zero problem inside a batch
    Z = Y.copy()
    Z[1] = 0
    xz = tw.wpe(Z, 3, 1, 2)
    assert (xz[1] == 0).all() and (xz[[0, 2]] == tw.wpe(Y[[0, 2]], 3, 1, 2)).all()
    with pytest.raises(AssertionError):
        tw.wpe(Y.real.copy(), 3, 1, 1)
    with pytest.raises(NotImplementedError, match='WPE_MAX_M = 96'):
        tw.wpe(np.zeros((8, 50), np.complex64), taps=13)
    with pytest.raises(NotImplementedError, match='WPE_MAX_D = 16'):
        tw.wpe(np.zeros((17, 50), np.complex64), taps=1)


def test_kinds_and_dtypes(tw):
    from pb_bss_amd import _lib
    t = _lib.torch()
    Y, want = reference((3, 3, 2, 65), 'complex64', 'full')
    for y in (Y, Y.astype(np.complex128), Y[0], Y.reshape(3, 1, 3, 65)):
        x = tw.wpe(y, 3, 2, 1)
        assert isinstance(x, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape
        assert (x.reshape(-1, 3, 65)[0] == tw.wpe(Y[0].astype(y.dtype), 3, 2, 1)).all()
    yd = t.from_numpy(Y.copy()).cuda()
    xd = tw.wpe(yd, 3, 2, 1)
    assert xd.is_cuda and xd.dtype == t.complex64 and (xd.cpu().numpy() == tw.wpe(Y, 3, 2, 1)).all()
    inv = tw.get_power_inverse(yd)
    R, P = tw.get_correlations(yd, inv, 3, 2)
    G = tw.get_filter_matrix(R, P)
    x = tw.perform_filter_operation(yd, G, 3, 2)
    assert inv.dtype == t.float64 and R.dtype == P.dtype == G.dtype == t.complex128
    assert all(a.is_cuda for a in (inv, R, P, G, x)) and x.dtype == t.complex64
    assert bool((x == xd).all())   # the parts run the kernels of the one-call path


def test_raw_c_abi_refuses_bad_arguments(tw):
    from pb_bss_amd import _lib
    t = _lib.torch()
    lib, h = _lib.load(), _lib.handle(0)
    B, D, T, taps = 2, 4, 40, 3
    M = D * taps
    y = t.ones((B, D, T), dtype=t.complex128, device='cuda')
    x = t.full((B, D, T), 7.0, dtype=t.complex128, device='cuda')
    st = t.full((B,), 7, dtype=t.int32, device='cuda')
    inv = t.ones((B, T), dtype=t.float64, device='cuda')
    R = t.full((B, M, M), 7.0, dtype=t.complex128, device='cuda')
    P = t.full((B, M, D), 7.0, dtype=t.complex128, device='cuda')
    G = t.full((B, M, D), 7.0, dtype=t.complex128, device='cuda')
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED

    def whole(y_=y, taps_=taps, delay=2, its=1, ctx=0, mode=0, x_=x, st_=st, D_=D):
        return lib.pbbss_wpe(h, p(y_) if y_ is not None else None, 1, B, D_, T, D_ * T, T, 1,
                             taps_, delay, its, ctx, mode, p(x_) if x_ is not None else None,
                             p(st_) if st_ is not None else None, None)
    assert whole(y_=None) == INV and whole(x_=None) == INV and whole(st_=None) == INV
    assert whole(taps_=0) == INV and whole(delay=-1) == INV and whole(mode=2) == INV
    assert whole(its=0) == INV and whole(ctx=-2) == INV
    assert whole(taps_=25) == UNS                       # M = 100
    assert lib.pbbss_wpe(h, p(y), 1, 1, 17, 4, 68, 4, 1, 1, 1, 1, 0, 0, p(x), p(st), None) == UNS

    def corr(taps_=taps, delay=2, mode=0, inv_=inv):
        return lib.pbbss_wpe_correlations(h, p(y), 1, B, D, T, D * T, T, 1,
                                          p(inv_) if inv_ is not None else None, taps_, delay, mode,
                                          p(R), p(P), None)
    assert corr(inv_=None) == INV and corr(taps_=0) == INV and corr(delay=-1) == INV
    assert corr(mode=-1) == INV and corr(taps_=25) == UNS

    def apply(taps_=taps, delay=2, G_=G):
        return lib.pbbss_wpe_apply_filter(h, p(y), 1, B, D, T, D * T, T, 1,
                                          p(G_) if G_ is not None else None, taps_, delay, p(x), None)
    assert apply(G_=None) == INV and apply(taps_=0) == INV and apply(delay=-1) == INV
    assert apply(taps_=25) == UNS
    assert lib.pbbss_wpe_filter_matrix(h, p(R), p(P), B, D, 25, p(G), p(st), None) == UNS
    assert lib.pbbss_wpe_filter_matrix(h, None, p(P), B, D, taps, p(G), p(st), None) == INV
    assert lib.pbbss_wpe_power_inverse(h, p(y), 1, B, D, T, D * T, T, 1, -2, p(inv), None, None) == INV
    t.cuda.synchronize()
    for a in (x, R, P, G):
        assert bool((a == 7.0).all())
    assert bool((st == 7).all()) and bool((inv == 1.0).all())
