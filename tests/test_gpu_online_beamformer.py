"""GPU: the frame-recursive MVDR beamformer (csrc/online_bf.hip;
pb_bss_amd.extraction.recursive_mvdr_souden, OnlineMVDR) against the NumPy restatement
tests/oracle_online_beamformer.py.

E_CASE is the restatement's own error (float64 run against the longdouble run, relative to
max |X|, max |W|, max |Phi| and max |Psi|) for exactly the inputs of the sweep, the larger of both
input dtypes; tests/test_online_beamformer_oracle.py re-measures it and keeps this copy within a
factor of 4.  The device bound of a case is 16 * max(e_case, 1e-13) relative to the maximum of the
quantity, with the constants and the reasoning of tests/test_gpu_wpe_online.py: the floor is about
T eps for the longest row, 16 leaves room for another summation order (the device adds its dot
products on fixed lane trees, multiplies by 1 / alpha and by 1 / max(lam, tiny) where NumPy
divides).  complex64 output adds half an ulp of complex64 of max |X| per component and is compared
with the restatement rounded the same way.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle_online_beamformer as oo

pytestmark = pytest.mark.gpu

E_CASE = {
    ((1, 8), 1.0): (1.7e-16, 1.1e-16, 1.5e-16, 2.6e-16),
    ((1, 8), 0.999): (9.7e-17, 1.1e-16, 7.4e-17, 1.3e-15),
    ((1, 8), 0.95): (1.7e-16, 1.1e-16, 1.4e-16, 7.7e-16),
    ((2, 64), 1.0): (1.3e-15, 3.2e-15, 2.1e-16, 4.8e-16),
    ((2, 64), 0.999): (1.2e-15, 2.9e-15, 1.9e-16, 3.1e-15),
    ((2, 64), 0.95): (2.0e-15, 3.2e-15, 2.3e-16, 3.0e-15),
    ((3, 65), 1.0): (2.2e-15, 3.4e-15, 4.1e-16, 2.9e-16),
    ((3, 65), 0.999): (2.5e-15, 4.9e-15, 4.3e-16, 3.5e-15),
    ((3, 65), 0.95): (1.5e-15, 3.9e-15, 8.9e-17, 2.7e-15),
    ((4, 130), 1.0): (1.7e-15, 2.2e-15, 2.3e-16, 2.4e-16),
    ((4, 130), 0.999): (1.9e-15, 3.1e-15, 3.4e-16, 7.5e-15),
    ((4, 130), 0.95): (2.2e-15, 2.5e-15, 2.0e-16, 2.9e-15),
    ((5, 33), 1.0): (2.7e-15, 2.1e-15, 2.9e-16, 5.7e-16),
    ((5, 33), 0.999): (1.4e-15, 2.2e-15, 3.4e-16, 2.5e-15),
    ((5, 33), 0.95): (2.4e-15, 2.9e-15, 2.9e-16, 2.0e-15),
    ((8, 300), 1.0): (1.4e-15, 2.8e-15, 6.0e-16, 7.9e-16),
    ((8, 300), 0.999): (2.2e-15, 3.2e-15, 6.4e-16, 1.3e-14),
    ((8, 300), 0.95): (2.3e-15, 5.1e-15, 2.2e-16, 3.7e-15),
    ((16, 200), 1.0): (3.1e-15, 5.1e-15, 5.4e-16, 1.0e-15),
    ((16, 200), 0.999): (5.2e-15, 6.7e-15, 1.2e-15, 9.9e-15),
    ((16, 200), 0.95): (4.9e-15, 1.1e-14, 2.8e-16, 4.3e-15),
    ((2, 1000), 1.0): (2.2e-15, 4.3e-15, 1.3e-15, 1.4e-15),
    ((2, 1000), 0.999): (2.0e-15, 3.3e-15, 1.5e-15, 4.2e-14),
    ((2, 1000), 0.95): (6.9e-16, 1.8e-15, 3.7e-16, 2.2e-15),
    ((2, 31), 1.0): (5.5e-16, 7.1e-16, 1.4e-16, 2.6e-16),
    ((2, 31), 0.999): (1.0e-15, 8.1e-16, 2.5e-16, 1.6e-15),
    ((2, 31), 0.95): (7.1e-16, 1.0e-15, 2.6e-16, 1.5e-15),
    ((2, 32), 1.0): (5.3e-16, 1.5e-15, 8.3e-17, 2.4e-16),
    ((2, 32), 0.999): (7.0e-16, 1.9e-15, 2.7e-16, 1.9e-15),
    ((2, 32), 0.95): (7.2e-16, 2.7e-15, 1.3e-16, 1.4e-15),
    ((2, 33), 1.0): (2.0e-15, 3.6e-15, 3.0e-16, 9.2e-16),
    ((2, 33), 0.999): (2.3e-15, 8.1e-15, 4.5e-16, 2.1e-15),
    ((2, 33), 0.95): (2.5e-15, 4.6e-15, 3.0e-16, 1.5e-15),
    ((9, 70), 1.0): (8.1e-16, 2.7e-15, 2.3e-16, 7.2e-16),
    ((9, 70), 0.999): (8.2e-16, 3.2e-15, 4.3e-16, 4.3e-15),
    ((9, 70), 0.95): (7.3e-16, 3.9e-15, 4.1e-16, 3.4e-15),
    ((12, 70), 1.0): (1.6e-15, 3.5e-15, 4.2e-16, 6.2e-16),
    ((12, 70), 0.999): (2.6e-15, 4.8e-15, 6.2e-16, 4.1e-15),
    ((12, 70), 0.95): (2.9e-15, 6.4e-15, 2.1e-16, 3.5e-15),
}
EPS = 2.0 ** -52


@pytest.fixture(scope='module')
def ex():
    from pb_bss_amd import _lib
    from pb_bss_amd import extraction
    _lib.require_gpu()
    return extraction


@functools.lru_cache(maxsize=None)
def reference(case, alpha, dtype_name):
    """(Y (BATCH, D, T), target mask, noise mask, X, W, target_psd, noise_inv) of the
    restatement."""
    Y, s, v = oo.case_input(case, np.dtype(dtype_name))
    X, W, Phi, Psi, flagged = oo.recursive(Y, s, v, alpha, oo.ref_channel(case), oo.P0)
    assert not flagged.any()
    out = (Y, s, v, X, W, Phi, Psi)
    for a in out:
        a.setflags(write=False)
    return out


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


def same(a, b):
    """equal bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(ex, Y, s, v, alpha, ref, p0=oo.P0, **kw):
    """recursive_mvdr_souden on NumPy input -> (X, W, target_psd, noise_inv, state)."""
    X, W, st = ex.recursive_mvdr_souden(Y, s, v, alpha, ref, p0, return_state=True,
                                        return_vector=True, **kw)
    return X, W, host(st.target_psd), host(st.noise_inv), st


@pytest.mark.parametrize('alpha', oo.ALPHAS)
@pytest.mark.parametrize('case', oo.CASES, ids=str)
def test_parity(ex, case, alpha):
    D, T = case
    r = oo.ref_channel(case)
    worst = 0.0
    for dtype_name in ('complex128', 'complex64'):
        Y, s, v, Xw, Ww, Phiw, Psiw = reference(case, alpha, dtype_name)
        for B in (1, oo.BATCH):
            X, W, Phi, Psi, st = run(ex, Y[:B], s[:B], v[:B], alpha, r)
            assert X.dtype == Y.dtype and X.shape == (B, T)
            assert W.shape == (T, B, D) and Phi.shape == Psi.shape == (B, D, D)
            assert W.dtype == Phi.dtype == Psi.dtype == np.complex128
            assert (host(st.frames_seen) == T).all() and (host(st.status) == 0).all()
            for M in (Phi, Psi):
                assert (M == M.conj().swapaxes(-1, -2)).all()       # Hermitian to the bit
                assert (np.diagonal(M, axis1=-2, axis2=-1).imag == 0).all()
            assert (W[0] == 0).all() and (X[:, 0] == 0).all()       # Phi is still 0
            for name, got, want, e in zip(('X', 'W', 'Phi', 'Psi'), (X, W, Phi, Psi),
                                          (Xw[:B], Ww[:, :B], Phiw[:B], Psiw[:B]),
                                          E_CASE[case, alpha]):
                err, ulp = distance(got, want)
                bound = 16 * max(e, 1e-13) + ulp
                print(f'{case} a={alpha} {dtype_name} B={B} {name}: {err:.2e} (bound {bound:.2e})')
                worst = max(worst, (err - ulp) / (16 * max(e, 1e-13)))
                assert err <= bound, (case, alpha, dtype_name, B, name, err, bound)
    print(f'{case} a={alpha}: worst {worst:.3f} of the bound')


@pytest.mark.parametrize('alpha', oo.ALPHAS)
@pytest.mark.parametrize('case', [(2, 64), (4, 130), (8, 300), (12, 70), (16, 200), (2, 1000)],
                         ids=str)
def test_last_vector_is_the_batch_souden_solution_of_the_devices_own_statistics(ex, case, alpha):
    r = oo.ref_channel(case)
    Y, s, v = reference(case, alpha, 'complex128')[:3]
    _, W, Phi, Psi, _ = run(ex, Y, s, v, alpha, r)
    N = np.linalg.inv(Psi)
    want = ex.get_mvdr_vector_souden(Phi, N, ref_channel=r)
    for b in range(oo.BATCH):
        cond = np.linalg.cond(Psi[b])
        err, tol = np.abs(W[-1, b] - want[b]).max(), 16 * cond * EPS * np.abs(want[b]).max()
        print(f'{case} a={alpha} b={b}: {err:.2e} (tol {tol:.2e}, cond {cond:.1e})')
        assert err <= tol, (case, alpha, b, err, tol, cond)


@pytest.mark.parametrize('case', [(2, 130), (16, 100)], ids=str)
def test_blocking_is_bitwise_invisible(ex, case):
    from pb_bss_amd import _lib
    t = _lib.torch()
    D, T = case
    alpha, r = 0.95, oo.ref_channel(case)
    Y, s, v = oo.case_input(case, np.complex64)
    X, W, Phi, Psi, _ = run(ex, Y, s, v, alpha, r)

    def in_blocks(lengths):
        st, xs, ws, t0 = None, [], [], 0
        for n in lengths:
            x, w, st = ex.recursive_mvdr_souden(
                Y[:, :, t0:t0 + n], s[:, t0:t0 + n], v[:, t0:t0 + n], alpha, r, oo.P0, state=st,
                return_state=True, return_vector=True)
            xs.append(x)
            ws.append(w)
            t0 += n
        assert t0 == T
        assert same(np.concatenate(xs, axis=-1), X) and same(np.concatenate(ws, axis=0), W)
        assert same(host(st.target_psd), Phi) and same(host(st.noise_inv), Psi)
        assert (host(st.frames_seen) == T).all()
    in_blocks([1] * T)
    in_blocks([1, 1, 7, 64, T - 73])     # 9 + 64 straddles two tile edges
    in_blocks([31, 2, 31, T - 64])
    # OnlineMVDR frame by frame and in blocks, in the (F, Tb, D) layout of OnlineWPE
    by_frame = ex.OnlineMVDR(D, oo.BATCH, alpha, r, oo.P0)
    assert by_frame.status is None and by_frame.vector is None
    frames = [by_frame.step_frame(Y[:, :, i], s[:, i], v[:, i]) for i in range(T)]
    assert frames[0].shape == (oo.BATCH,) and isinstance(frames[0], np.ndarray)
    assert same(np.stack(frames, axis=-1), X)
    assert same(host(by_frame.target_psd), Phi) and same(host(by_frame.noise_inv), Psi)
    assert same(host(by_frame.vector), W[-1]) and (host(by_frame.status) == 0).all()
    by_block = ex.OnlineMVDR(D, oo.BATCH, alpha, r, oo.P0)
    Yd = t.from_numpy(np.ascontiguousarray(Y.swapaxes(1, 2))).cuda()       # (F, T, D)
    sd, vd = t.from_numpy(s).cuda(), t.from_numpy(v).cuda()
    blocks = [by_block.step_block(Yd[:, a:b], sd[:, a:b], vd[:, a:b])
              for a, b in ((0, 33), (33, 34), (34, T))]
    assert all(x.is_cuda and x.dtype == t.complex64 for x in blocks)
    assert same(host(t.cat(blocks, dim=1)), X)
    assert same(host(by_block.target_psd), Phi) and same(host(by_block.noise_inv), Psi)
    assert same(host(by_block.vector), W[-1])


def test_determinism_and_batch_independence(ex):
    case, alpha = (8, 300), 0.999
    r = oo.ref_channel(case)
    Y, s, v = reference(case, alpha, 'complex64')[:3]
    Y5 = np.concatenate([Y, Y[:2] * 0.5 + Y[1:] * 0.25])
    s5, v5 = np.concatenate([s, s[:2]]), np.concatenate([v, v[1:]])
    a = run(ex, Y5, s5, v5, alpha, r)
    again = run(ex, Y5, s5, v5, alpha, r)
    assert all(same(a[i], again[i]) for i in range(4))
    for b in range(5):
        one = run(ex, Y5[b], s5[b], v5[b], alpha, r)
        assert one[0].shape == (300,) and one[1].shape == (300, 8)
        assert same(a[0][b], one[0]) and same(a[1][:, b], one[1]), b
        assert same(a[2][b], one[2][0]) and same(a[3][b], one[3][0]), b


@pytest.mark.parametrize('case', [(3, 65), (8, 300), (16, 200)], ids=str)
def test_the_vectors_reproduce_the_output(ex, case):
    """apply_online_beamforming_vector(W, Y) is the same D-term dot product summed in another
    order: within 8 D eps of max |X|."""
    D, T = case
    Y, s, v = reference(case, 0.999, 'complex128')[:3]
    X, W = run(ex, Y, s, v, 0.999, oo.ref_channel(case))[:2]
    again = ex.apply_online_beamforming_vector(W, Y)
    err, tol = np.abs(again - X).max(), 8 * D * EPS * np.abs(X).max()
    print(f'{case}: {err:.2e} (tol {tol:.2e})')
    assert again.shape == X.shape and err <= tol, (case, err, tol)


def test_layout_and_chain_behind_online_wpe(ex):
    from pb_bss_amd import _lib, transform
    t = _lib.torch()
    case, alpha = (4, 130), 0.95
    r = oo.ref_channel(case)
    Y, s, v = reference(case, alpha, 'complex64')[:3]
    X, W, Phi, Psi, _ = run(ex, Y, s, v, alpha, r)
    # (..., T, D) in memory
    a = run(ex, np.ascontiguousarray(Y.swapaxes(-1, -2)), s, v, alpha, r, layout='f t d')
    assert all(same(a[i], (X, W, Phi, Psi)[i]) for i in range(4))
    # a non-contiguous (..., T, D) view of (..., D, T) memory, as a tensor
    yd = t.from_numpy(Y.copy()).cuda()
    view = yd.transpose(1, 2)
    assert not view.is_contiguous()
    xv, wv = ex.recursive_mvdr_souden(view, s, v, alpha, r, oo.P0, layout='f t d',
                                      return_vector=True)
    assert xv.is_cuda and same(host(xv), X) and same(host(wv), W)
    with pytest.raises(ValueError):
        ex.recursive_mvdr_souden(Y, s, v, alpha, r, layout='t f d')
    # OnlineWPE.step_block -> OnlineMVDR.step_block: same shapes, no transpose, no copy
    F, D, T = Y.shape
    wpe = transform.OnlineWPE(taps=3, delay=2, alpha=0.999, channel=D, frequency_bins=F)
    mvdr = ex.OnlineMVDR(D, F, alpha, r, oo.P0)
    block = t.from_numpy(np.ascontiguousarray(Y.swapaxes(1, 2))).cuda()
    dry = wpe.step_block(block)
    assert dry.is_cuda and dry.is_contiguous() and dry.shape == (F, T, D)
    out = mvdr.step_block(dry, t.from_numpy(s).cuda(), t.from_numpy(v).cuda())
    assert out.is_cuda and out.shape == (F, T) and out.dtype == t.complex64
    want = ex.recursive_mvdr_souden(host(dry), s, v, alpha, r, oo.P0, layout='f t d')
    assert np.isfinite(want).all() and same(host(out), want)


def test_edges(ex):
    from pb_bss_amd import _lib
    t = _lib.torch()
    case, alpha = (3, 65), 0.95
    r = oo.ref_channel(case)
    Y, s, v, Xw, Ww, Phiw, Psiw = reference(case, alpha, 'complex128')
    X, W, Phi, Psi, st = run(ex, Y, s, v, alpha, r)
    # T = 0: empty output, the state unchanged
    X0, W0, st0 = ex.recursive_mvdr_souden(Y[:, :, :0], s[:, :0], v[:, :0], alpha, r, oo.P0,
                                           state=st, return_state=True, return_vector=True)
    assert X0.shape == (oo.BATCH, 0) and W0.shape == (0, oo.BATCH, 3) and X0.dtype == Y.dtype
    assert same(host(st0.noise_inv), Psi) and (host(st0.frames_seen) == 65).all()
    X0, st0 = ex.recursive_mvdr_souden(Y[:, :, :0], s[:, :0], v[:, :0], alpha, r, oo.P0,
                                       return_state=True)
    assert (host(st0.noise_inv) == np.eye(3) / oo.P0).all() and (host(st0.target_psd) == 0).all()
    assert (host(st0.frames_seen) == 0).all() and st0.status is None
    o = ex.OnlineMVDR(3, oo.BATCH, alpha, r, oo.P0)
    assert o.step_block(np.zeros((oo.BATCH, 0, 3), np.complex64), s[:, :0], v[:, :0]).shape == (
        oo.BATCH, 0)
    # D = 1, a single problem without a leading axis
    Y1, s1, v1, X1w, W1w = reference((1, 8), 0.95, 'complex128')[:5]
    x1, w1 = ex.recursive_mvdr_souden(Y1[0], s1[0], v1[0], 0.95, 0, oo.P0, return_vector=True)
    assert x1.shape == (8,) and w1.shape == (8, 1)
    assert np.abs(x1 - X1w[0]).max() <= 16e-13 * np.abs(X1w[0]).max()
    # float32 masks are widened, not rounded again: the float64 run on the same values
    s32, v32 = s.astype(np.float32), v.astype(np.float32)
    a = run(ex, Y, s32, v32, alpha, r)
    b = run(ex, Y, s32.astype(np.float64), v32.astype(np.float64), alpha, r)
    mixed = run(ex, Y, s32, v32.astype(np.float64), alpha, r)
    assert all(same(a[i], b[i]) and same(a[i], mixed[i]) for i in range(4))
    # tensor in, tensor out, without a host synchronisation; a continued state is not modified
    yd, sd, vd = (t.from_numpy(np.array(a)).cuda() for a in (Y, s, v))
    t.cuda.synchronize()
    t.cuda.set_sync_debug_mode('error')
    try:
        xd, wd, std = ex.recursive_mvdr_souden(yd, sd, vd, alpha, r, oo.P0, return_state=True,
                                               return_vector=True)
        keep = std.clone()
        x2, st2 = ex.recursive_mvdr_souden(yd, sd, vd, alpha, r, state=std, return_state=True)
    finally:
        t.cuda.set_sync_debug_mode('default')
    assert xd.is_cuda and wd.is_cuda and xd.dtype == t.complex128 and wd.dtype == t.complex128
    assert same(host(xd), X) and same(host(wd), W)
    assert all(a.is_cuda for a in (std.target_psd, std.noise_inv, std.frames_seen, std.status))
    assert std.frames_seen.dtype == t.int64 and std.status.dtype == t.int32
    for before, after in ((keep.target_psd, std.target_psd), (keep.noise_inv, std.noise_inv),
                          (keep.frames_seen, std.frames_seen)):
        assert bool((before == after).all())
    assert (host(st2.frames_seen) == 130).all() and not same(host(st2.noise_inv), Psi)
    # an inf sample in frame k of one problem of a batch
    k = 40
    N = Y.copy()
    N[1, 2, k] = np.inf
    Xn, Wn, Phin, Psin, stn = run(ex, N, s, v, alpha, r)
    assert host(stn.status).tolist() == [0, _lib.ST_NONFINITE, 0]
    assert same(Xn[1, :k], X[1, :k]) and same(Wn[:k, 1], W[:k, 1])
    assert np.isnan(Xn[1, k:]).all() and np.isnan(Wn[k:, 1]).all()
    assert np.isnan(Phin[1]).all() and np.isnan(Psin[1]).all()
    for got, clean in ((Xn, X), (Phin, Phi), (Psin, Psi)):
        assert same(got[[0, 2]], clean[[0, 2]])
    assert same(Wn[:, [0, 2]], W[:, [0, 2]])
    o = ex.OnlineMVDR(3, oo.BATCH, alpha, r, oo.P0)
    o.step_block(np.ascontiguousarray(N.swapaxes(1, 2)), s, v)
    assert host(o.status).tolist() == [0, _lib.ST_NONFINITE, 0]
    # all-zero masks: x = 0 and no flag at alpha = 1
    Xz, Wz, Phiz, Psiz, stz = run(ex, Y, 0 * s, 0 * v, 1.0, r)
    assert (Xz == 0).all() and (Wz == 0).all() and (Phiz == 0).all()
    assert (Psiz == np.eye(3) / oo.P0).all() and (host(stz.status) == 0).all()


def test_refusals(ex):
    Y, s, v = oo.case_input((3, 65))
    with pytest.raises(NotImplementedError, match='ONLINE_BF_MAX_D = 16'):
        ex.recursive_mvdr_souden(np.zeros((17, 50), np.complex64), np.zeros(50), np.zeros(50))
    with pytest.raises(NotImplementedError, match='ONLINE_BF_MAX_D = 16'):
        ex.OnlineMVDR(channel=17, frequency_bins=4)
    with pytest.raises(NotImplementedError, match='ONLINE_BF_MAX_D = 16'):
        ex.OnlineBeamformerState.initial(2, 17, 1.0)
    for alpha in (0.0, -0.5, 1.5, float('nan')):
        with pytest.raises(AssertionError):
            ex.recursive_mvdr_souden(Y, s, v, alpha=alpha)
    for ref in (-1, 3):
        with pytest.raises(AssertionError):
            ex.recursive_mvdr_souden(Y, s, v, ref_channel=ref)
    for p0 in (0.0, -1.0):
        with pytest.raises(AssertionError):
            ex.recursive_mvdr_souden(Y, s, v, initial_noise_power=p0)
    with pytest.raises(AssertionError):
        ex.recursive_mvdr_souden(Y.real.copy(), s, v)
    with pytest.raises(AssertionError):
        ex.recursive_mvdr_souden(Y, s.astype(np.float16), v)
    with pytest.raises(AssertionError):
        ex.OnlineMVDR(channel=4, frequency_bins=4, ref_channel=4)


def test_raw_c_abi_refuses_bad_arguments(ex):
    from pb_bss_amd import _lib
    t = _lib.torch()
    lib, h = _lib.load(), _lib.handle(0)
    B, D, T = 2, 4, 40
    c128 = dict(dtype=t.complex128, device='cuda')
    y = t.ones((B, D, T), **c128)
    x = t.full((B, T), 7.0, **c128)
    w = t.full((T, B, D), 7.0, **c128)
    Phi = t.full((B, D, D), 7.0, **c128)
    Psi = t.full((B, D, D), 7.0, **c128)
    seen = t.full((B,), 7, dtype=t.int64, device='cuda')
    st = t.full((B,), 7, dtype=t.int32, device='cuda')
    s = t.ones((B, T), dtype=t.float64, device='cuda')
    v = t.ones((B, T), dtype=t.float64, device='cuda')
    p = lambda a: ctypes.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED

    def call(y_=y, B_=B, D_=D, T_=T, s_=s, v_=v, alpha=0.99, ref=0, Phi_=Phi, Psi_=Psi,
             seen_=seen, x_=x, w_=w, st_=st):
        return lib.pbbss_online_mvdr(h, p(y_), 1, B_, D_, T_, D_ * T_, T_, 1, p(s_), p(v_), 1,
                                     alpha, ref, p(Phi_), p(Psi_), p(seen_), p(x_), p(w_), p(st_),
                                     None)
    for name in ('y_', 's_', 'v_', 'Phi_', 'Psi_', 'seen_', 'x_', 'st_'):
        assert call(**{name: None}) == INV, name
    for name in ('B_', 'D_', 'T_'):
        assert call(**{name: 0}) == INV, name
    for alpha in (0.0, -0.5, 1.0 + 2.0 ** -52, float('nan'), float('inf')):
        assert call(alpha=alpha) == INV, alpha
    assert call(ref=-1) == INV and call(ref=D) == INV
    assert call(D_=17, T_=1, B_=1) == UNS and call(D_=17, T_=1, B_=1, ref=16) == UNS
    assert call(D_=17, T_=1, B_=1, ref=17) == INV
    assert lib.pbbss_online_mvdr(None, p(y), 1, B, D, T, D * T, T, 1, p(s), p(v), 1, 0.99, 0,
                                 p(Phi), p(Psi), p(seen), p(x), p(w), p(st), None) == INV
    t.cuda.synchronize()
    for a in (x, w, Phi, Psi):
        assert bool((a == 7.0).all())
    assert bool((st == 7).all()) and bool((seen == 7).all())
    # a valid call: out_w may be null
    Phi.zero_()
    Psi.copy_(t.eye(D, **c128))
    seen.zero_()
    assert call(w_=None) == _lib.OK
    t.cuda.synchronize()
    assert bool((seen == T).all()) and bool((st == 0).all()) and bool((w == 7.0).all())
    assert bool(t.isfinite(t.view_as_real(x)).all())
