"""GPU: pb_bss_amd.initializer -- the device deflation seed (csrc/initializer.hip) against the
reference's recorded results (tests/golden/initializer_deflation_*.npz) and the float64
restatement (tests/oracle_initializer.py), the i.i.d. initialisers in 'device' mode, and the
hand-over of a device seed to the trainers.

Tolerance of the seed: max-abs 1e-10 on the posteriors, the project's figure for one-shot
float64 linear algebra.  The comparison presupposes that every arg-max and every dominant
eigenvector of the run is well determined; each test asserts that on the oracle side first
(oracle_initializer.assert_well_determined).
"""
import ctypes
import glob
import os

import numpy as np
import pytest

import oracle_initializer as oi

pytestmark = pytest.mark.gpu

TOL = 1e-10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEFLATION = sorted(glob.glob(os.path.join(GOLDEN, 'initializer_deflation_*.npz')))


def torch():
    import torch as t
    return t


def seed_fn():
    from pb_bss_amd.initializer.deflation import deflationSeed
    return deflationSeed


def host(x):
    return x.detach().cpu().numpy() if not isinstance(x, np.ndarray) else x


def check_properties(post, Y, K):
    """what every seed must satisfy, whatever the input"""
    post = host(post)
    Y = host(Y)
    assert post.shape == (*Y.shape[:-3], K, *Y.shape[-3:-1]) and post.dtype == np.float64
    assert np.isfinite(post).all()
    assert (post >= 0).all()
    assert np.abs(post.sum(-3) - 1).max() <= 1e-14
    silent = np.moveaxis((np.abs(Y) ** 2).sum(-1) == 0, (-2, -1), (-2, -1))  # (..., F, T)
    last = np.zeros(K)
    last[-1] = 1
    got = np.moveaxis(post, -3, -1)[silent]  # (n, K)
    assert (got == last).all()


def oracle(Y, K, **kw):
    details = {}
    ref = oi.deflation_seed(Y, K, details=details, **kw)
    oi.assert_well_determined(details)
    return ref, details


def compare(post, ref, what):
    err = float(np.abs(host(post) - ref).max())
    print(f'{what}: max-abs {err:.2e}')
    assert err <= TOL, (what, err)


@pytest.mark.parametrize('path', DEFLATION, ids=[os.path.basename(p)[:-4] for p in DEFLATION])
@pytest.mark.parametrize('pf', [True, False])
@pytest.mark.parametrize('dtype', [np.complex64, np.complex128])
def test_fixtures(path, pf, dtype):
    g = np.load(path)
    F, T, D, K, seed, nb = (int(g[k]) for k in ('F', 'T', 'D', 'K', 'seed', 'neighbors'))
    Y = oi.synth_case(F, T, D, K, seed).astype(dtype)
    oracle(Y, K, permutation_free=pf, neighbors=nb)  # precondition
    ref = g[f'posterior_pf{int(pf)}']
    post = seed_fn()(Y, K, permutation_free=pf, neighbors=nb)
    assert isinstance(post, np.ndarray)
    check_properties(post, Y, K)
    compare(post, ref, f'{os.path.basename(path)} pf={pf} {np.dtype(dtype).name} numpy')
    Yd = torch().from_numpy(Y).cuda()
    postd = seed_fn()(Yd, K, permutation_free=pf, neighbors=nb)
    assert postd.is_cuda and postd.dtype == torch().float64
    assert np.array_equal(host(postd), post)


@pytest.mark.parametrize('shape', [(513, 500, 8, 3), (257, 800, 6, 3)])
@pytest.mark.parametrize('pf', [True, False])
@pytest.mark.parametrize('dtype', [np.complex64, np.complex128])
def test_full_size(shape, pf, dtype):
    from pb_bss_amd import engine
    F, T, D, K = shape
    Y = oi.synth_case(F, T, D, K, 0).astype(dtype)
    ref, details = oracle(Y, K, permutation_free=pf)
    Yd = torch().from_numpy(Y).cuda()
    post = seed_fn()(Yd, K, permutation_free=pf)
    check_properties(post, Y, K)
    compare(post, ref, f'{shape} pf={pf} {np.dtype(dtype).name}')
    _, peak = engine.deflation_seed(Yd[None], K, permutation_free=pf, want_peak=True)
    peak = host(peak)[0]
    if pf:  # one peak frame per utterance and round
        assert (peak == peak[:, :1]).all()
    nonzero = np.abs(Y).sum((1, 2)) > 0
    assert np.array_equal(peak[:, nonzero], details['peaks'][:, nonzero])
    # an all-zero bin: arg-max 0, clipped to `neighbors`
    if not pf:
        assert (peak[:, ~nonzero] == 5).all()


@pytest.mark.parametrize('D', [2, 3, 4, 5, 6, 7, 8, 12])
@pytest.mark.parametrize('pf', [True, False])
def test_sensor_counts(D, pf):
    F, T, K = 257, 72, 3
    for dtype in (np.complex64, np.complex128):
        Y = oi.synth_case(F, T, D, K, 30 + D).astype(dtype)
        ref, _ = oracle(Y, K, permutation_free=pf)
        post = seed_fn()(Y, K, permutation_free=pf)
        check_properties(post, Y, K)
        compare(post, ref, f'D={D} pf={pf} {np.dtype(dtype).name}')


@pytest.mark.parametrize('K', [2, 3, 4, 6])
@pytest.mark.parametrize('pf', [True, False])
def test_class_counts(K, pf):
    F, T, D = 257, 90, 5
    Y = oi.synth_case(F, T, D, K, 50 + K)
    ref, _ = oracle(Y, K, permutation_free=pf, neighbors=4)
    post = seed_fn()(Y, K, permutation_free=pf, neighbors=4)
    check_properties(post, Y, K)
    compare(post, ref, f'K={K} pf={pf}')


@pytest.mark.parametrize('pf', [True, False])
def test_caller_saliencies_transform_and_eps(pf):
    F, T, D, K = 257, 80, 4, 3
    Y = oi.synth_case(F, T, D, K, 61)
    rng = np.random.default_rng(7)
    given = rng.uniform(0.1, 1.0, size=(F, T)) * np.linalg.norm(Y.astype(np.complex128), axis=-1)

    def soften(similarity, saliencies):
        assert type(similarity) is type(saliencies)
        return similarity ** 2

    for kw in (dict(saliencies=given), dict(eps=1e-3), dict(similarity_transform=soften),
               dict(saliencies=given, similarity_transform=soften, eps=1e-2)):
        ref, _ = oracle(Y, K, permutation_free=pf, **kw)
        post = seed_fn()(Y, K, permutation_free=pf, **kw)
        assert isinstance(post, np.ndarray)
        compare(post, ref, f'pf={pf} {sorted(kw)}')
        if 'eps' not in kw:
            check_properties(post, Y, K)
        dkw = dict(kw)
        if 'saliencies' in dkw:
            dkw['saliencies'] = torch().from_numpy(given).cuda()
        postd = seed_fn()(torch().from_numpy(Y).cuda(), K, permutation_free=pf, **dkw)
        assert postd.is_cuda and np.array_equal(host(postd), post)


@pytest.mark.parametrize('pf', [True, False])
def test_batch_equals_single_calls_bit_for_bit(pf):
    F, T, D, K = 257, 100, 6, 3
    Ys = np.stack([oi.synth_case(F, T, D, K, 70 + u, zero_bin=3 + u) for u in range(4)])
    for u in range(4):
        ref, _ = oracle(Ys[u], K, permutation_free=pf)
    Yd = torch().from_numpy(Ys).cuda()
    batch = seed_fn()(Yd, K, permutation_free=pf)
    assert tuple(batch.shape) == (4, K, F, T)
    check_properties(batch, Ys, K)
    for u in range(4):
        single = seed_fn()(Yd[u], K, permutation_free=pf)
        assert torch().equal(batch[u], single), u
    compare(batch[3], ref, f'batch member 3 pf={pf}')
    nested = seed_fn()(Yd.reshape(2, 2, F, T, D), K, permutation_free=pf)
    assert torch().equal(nested.reshape(4, K, F, T), batch)


@pytest.mark.parametrize('pf', [True, False])
def test_raw_c_abi(pf):
    from pb_bss_amd import _lib
    t = torch()
    F, T, D, K = 257, 64, 4, 3
    Y = oi.synth_case(F, T, D, K, 21)
    ref, details = oracle(Y, K, permutation_free=pf)
    lib = _lib.load()
    y = t.from_numpy(Y).cuda().contiguous()
    out = t.empty((1, K, F, T), dtype=t.float64, device='cuda')
    peak = t.empty((1, K - 1, F), dtype=t.int32, device='cuda')
    h = _lib.handle(0)
    stream = _lib.stream_ptr(0)

    def call(**over):
        a = dict(B=1, F=F, T=T, D=D, K=K, nb=5, r0=0, r1=K - 1, fin=1, state=None)
        a.update(over)
        return lib.pbbss_deflation_seed(
            h, _lib.ptr(y), 0, a['B'], a['F'], a['T'], a['D'], a['K'], None, int(pf), a['nb'], 0.0,
            a['r0'], a['r1'], a['fin'], _lib.ptr(a['state']), _lib.ptr(out), _lib.ptr(peak), stream)

    assert call() == _lib.OK
    t.cuda.synchronize()
    compare(out[0], ref, f'C ABI pf={pf}')
    nonzero = np.abs(Y).sum((1, 2)) > 0
    assert np.array_equal(host(peak)[0][:, nonzero], details['peaks'][:, nonzero])
    # error model: integer codes, nothing launched
    assert call(K=1) == _lib.ERR_UNSUPPORTED and call(K=20) == _lib.ERR_UNSUPPORTED
    assert call(D=1) == _lib.ERR_UNSUPPORTED and call(D=33) == _lib.ERR_UNSUPPORTED
    assert call(nb=32) == _lib.ERR_INVALID_ARG          # T <= 2 neighbors
    assert call(r1=K) == _lib.ERR_INVALID_ARG
    assert call(r1=1, fin=0) == _lib.ERR_INVALID_ARG    # a partial call needs the state array
    assert call(B=0) == _lib.ERR_INVALID_ARG
    t.cuda.synchronize()
    from pb_bss_amd import engine
    with pytest.raises(NotImplementedError):
        engine.deflation_seed(y[None], 20)


def test_long_utterances_leave_lds():
    """frames that do not fit LDS are read in place; a saliency row that does not fit lives in
    the state array"""
    for (F, T, D, K, dtype) in [(257, 1500, 8, 3, np.complex128), (257, 21000, 2, 2, np.complex64)]:
        Y = oi.synth_case(F, T, D, K, 80 + D).astype(dtype)
        for pf in (False, True):
            ref, _ = oracle(Y, K, permutation_free=pf)
            post = seed_fn()(torch().from_numpy(Y).cuda(), K, permutation_free=pf)
            check_properties(post, Y, K)
            compare(post, ref, f'T={T} D={D} pf={pf}')


@pytest.mark.parametrize('pf', [True, False])
def test_captured_and_replayed(pf):
    from pb_bss_amd.pipeline import graphed
    t = torch()
    F, T, D, K = 257, 96, 6, 3
    Ya = oi.synth_case(F, T, D, K, 24)
    Yb = oi.synth_case(F, T, D, K, 25)
    fn = lambda y: seed_fn()(y, K, permutation_free=pf)  # noqa: E731
    g = graphed(fn, t.from_numpy(Ya).cuda())
    assert g.captured
    for Y in (Yb, Ya):
        ref, _ = oracle(Y, K, permutation_free=pf)
        yd = t.from_numpy(Y).cuda()
        post = g(yd).clone()
        t.cuda.synchronize()
        compare(post, ref, f'graph replay pf={pf}')
        assert t.equal(post, fn(yd))


def test_non_finite_input_raises_nothing():
    F, T, D, K = 257, 64, 4, 3
    Y = oi.synth_case(F, T, D, K, 21)
    clean = seed_fn()(Y, K, permutation_free=False)
    Y[7, 20, 1] = np.nan
    Y[9, 30, 0] = np.inf
    post = seed_fn()(Y, K, permutation_free=False)
    assert not np.isfinite(post[:, 7]).all() and not np.isfinite(post[:, 9]).all()
    others = [f for f in range(F) if f not in (7, 9)]
    assert np.array_equal(post[:, others], clean[:, others])
    post = seed_fn()(Y, K, permutation_free=True)
    assert post.shape == (K, F, T) and not np.isfinite(post[:, 7]).all()


def test_iid_device_mode():
    from pb_bss_amd.distribution.utils import random_init
    from pb_bss_amd.initializer import deterministic, iid
    t = torch()
    t.manual_seed(0)
    Y = t.ones((6, 5, 4000, 3), device='cuda')
    K = 4
    with random_init('device'):
        state = np.random.get_state()[1].copy()
        for name in iid.__all__:
            for pf in (False, True):
                a = getattr(iid, name)(Y, K, permutation_free=pf)
                assert a.is_cuda and a.dtype == t.float64 and tuple(a.shape) == (6, 5, K, 4000)
                assert float((a.sum(-2) - 1).abs().max()) <= 1e-14 and bool((a >= 0).all())
                if pf:
                    assert t.equal(a, a[0, 0].expand(a.shape))
                else:
                    assert not t.equal(a[0, 0], a[1, 0])
        assert np.array_equal(np.random.get_state()[1], state)  # NumPy's stream untouched
        hot = iid.one_hot(Y, K)
        assert bool(((hot == 0) | (hot == 1)).all()) and float(hot.sum(-2).min()) == 1.0
        # NumPy in, NumPy out -- drawn on the device all the same
        assert isinstance(iid.dirichlet(np.ones((2, 9, 3)), 3), np.ndarray)
        for alpha in (1, 0.5, 3.0):
            a = iid.dirichlet(Y, K, alpha=alpha)
            n = a.numel() // K
            flat = a.movedim(-2, 0).reshape(K, n)
            var = (K - 1) / (K ** 2 * (K * alpha + 1))
            # standard error of the sample mean / of the sample variance (fourth moment of a
            # Beta(alpha, (K-1) alpha) variable bounded by var: values lie in [0, 1])
            se_mean = (var / n) ** 0.5
            m4 = float(((flat - 1 / K) ** 4).mean())
            se_var = ((m4 - var ** 2) / n) ** 0.5
            for k in range(K):
                assert abs(float(flat[k].mean()) - 1 / K) <= 5 * se_mean, (alpha, k)
                assert abs(float(flat[k].var(unbiased=False)) - var) <= 5 * se_var, (alpha, k)
    f = deterministic.flag(Y, K, permutation_free=True, minimum=0.1)
    assert f.is_cuda and tuple(f.shape) == (6, 5, K, 4000)
    assert np.array_equal(host(f), deterministic.flag(np.ones((6, 5, 4000, 3)), K, True, 0.1))


def test_seed_view_feeds_the_trainers_without_a_host_round_trip():
    """CACGMMTrainer.fit from the transposed (non-contiguous) device view of a seed with exact
    zeros in it == the oracle EM started from the same array."""
    from oracle import cacgmm as oc
    from pb_bss_amd.distribution import CACGMMTrainer, CBMMTrainer, CWMMTrainer
    t = torch()
    F, T, D, K = 257, 120, 6, 3
    Y = oi.synth_case(F, T, D, K, 90, zero_bin=None, zero_tail=0)
    Yd = t.from_numpy(Y).cuda()
    seed = seed_fn()(Yd, K)
    view = seed.transpose(1, 0)  # (F, K, T)
    assert view.is_cuda and not view.is_contiguous()
    assert float(seed.min()) == 0.0  # the clipped last class
    model = CACGMMTrainer().fit(Yd, initialization=view, iterations=10)
    masks = host(model.predict(Yd))
    Y128 = Y.astype(np.complex128)
    ref = oc.em_predict(oc.em_fit(Y128, host(view), iterations=10), Y128)
    err = float(np.abs(masks - ref).max())
    print(f'CACGMM from the device seed vs oracle EM: {err:.2e}')
    assert err < 1e-8, err
    for trainer in (CWMMTrainer(), CBMMTrainer()):
        m = trainer.fit(Yd, initialization=view, iterations=2)
        p = m.predict(Yd)
        assert p.is_cuda and tuple(p.shape) == (F, K, T) and bool(t.isfinite(p).all())
