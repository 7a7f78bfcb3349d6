"""GPU: pb_bss_amd.distribution.kmeans (KMeans, BinaryGMM, BinaryGMMTrainer; csrc/kmeans.hip)
against the float64 restatement tests/oracle_kmeans.py.

Input condition, asserted on the restatement alone before anything is compared: the two nearest
centres of every row differ by more than 1e-9 relative (`margin`) and every drawn value of the
seeding is more than 1e-9 of the potential away from a prefix-sum boundary (`gap`).  The device's
distances and prefix sums differ from the restatement's by a few 1e-16 N relative (another order
of the same float64 sums), so under that condition every discrete decision -- labels, n_iter_,
seeding indices -- is the same and is compared exactly.

Tolerances: float64 centres 1e-10 absolute on unit-scale data (a centre is a sum of at most N
terms divided by a count: reordering costs about N 2^-53 <= 5e-11 relative for N <= 2^18);
float32-input centres one float32 ulp of the rounded restatement; inertia 1e-10 relative.
float32 input is compared with the restatement fed x.astype(float64).
"""
import functools

import numpy as np
import pytest

import oracle_kmeans as ok

pytestmark = pytest.mark.gpu

TOL = 1e-10
CONDITION = 1e-9


def _torch():
    import torch
    return torch


def km():
    from pb_bss_amd.distribution import kmeans
    return kmeans


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def check_centers(got, want, what):
    got, want = host(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.float32:
        rounded = want.astype(np.float32)
        ulps = np.abs(got - rounded) / np.spacing(np.abs(rounded))
        print(f'{what}: centres differ by at most {ulps.max():.2f} float32 ulp')
        assert ulps.max() <= 1.0, (what, ulps.max())
    else:
        assert got.dtype == np.float64, got.dtype
        worst = np.abs(got - want).max()
        print(f'{what}: largest centre difference {worst:.3e}')
        assert worst <= TOL, (what, worst)


def check_fit(model, ref, what, exact_ties=False):
    """model: a fitted KMeans of one problem; ref: what oracle_kmeans.lloyd returned.
    exact_ties: the case holds identical centres, whose distances are equal bit for bit on both
    sides (margin 0 by construction)."""
    assert exact_ties or ref['margin'] > CONDITION, (what, ref['margin'])
    labels = host(model.labels_)
    assert labels.dtype == np.int32
    assert int(host(model.n_iter_)) == ref['n_iter'], (what, model.n_iter_, ref['n_iter'])
    np.testing.assert_array_equal(labels, ref['labels'], err_msg=what)
    check_centers(model.cluster_centers_, ref['centers'], what)
    inertia = float(host(model.inertia_))
    rel = abs(inertia - ref['inertia']) / max(ref['inertia'], 1e-300) if ref['inertia'] else inertia
    print(f'{what}: inertia differs by {rel:.3e} relative')
    assert rel <= TOL, (what, inertia, ref['inertia'])


# ---- shapes: tile and chunk edges, every accumulation path --------------------------------------
# (B, N, E, K, dtype, max_iter)
SHAPES = [
    (1, 1, 1, 1, np.float64, 300),
    (1, 63, 7, 2, np.float32, 300),
    (3, 257, 40, 3, np.float32, 300),
    (1, 3001, 40, 8, np.float64, 300),
    (1, 4099, 7, 9, np.float32, 300),      # one class beyond the register path
    (1, 3001, 1, 17, np.float64, 300),
    (1, 257, 1, 64, np.float32, 300),
    (1, 4099, 256, 64, np.float64, 3),     # K E at its maximum
    (3, 63, 256, 2, np.float32, 300),
    (1, 257, 64, 8, np.float64, 300),      # the largest register-path shape
    (1, 257, 65, 8, np.float32, 300),      # one column beyond it
    (1, 4099, 40, 3, np.float32, 300),
]


@functools.lru_cache(maxsize=None)
def shape_case(i):
    B, N, E, K, dtype, max_iter = SHAPES[i]
    xs, inits, refs, seeds = [], [], [], []
    for b in range(B):
        x = ok.make_data(N, E, K, 100 + 10 * i + b).astype(dtype)
        wide = x.astype(np.float64)
        init = ok.initial_centers(wide, K, 100 + 10 * i + b)
        xs.append(x)
        inits.append(init)
        refs.append(ok.lloyd(wide, init, max_iter=max_iter))
        rnd = ok.draw_randoms(np.random.RandomState(200 + 10 * i + b), K)
        seeds.append((rnd, ok.kmeans_plusplus(wide, K, rnd)))
    return np.stack(xs), np.stack(inits), refs, seeds


def one_problem(model, b, batched):
    class View:
        pass
    v = View()
    for name in ('labels_', 'cluster_centers_', 'inertia_', 'n_iter_'):
        a = getattr(model, name)
        setattr(v, name, a[b] if batched else a)
    return v


@pytest.mark.parametrize('i', range(len(SHAPES)), ids=[
    f'B{s[0]}-N{s[1]}-E{s[2]}-K{s[3]}-{np.dtype(s[4]).name}' for s in SHAPES])
def test_shapes_fit_and_seeding(i):
    B, N, E, K, dtype, max_iter = SHAPES[i]
    x, init, refs, seeds = shape_case(i)
    batched = B > 1
    xin, cin = (x, init) if batched else (x[0], init[0])
    model = km().KMeans(n_clusters=K, init=cin, max_iter=max_iter).fit(xin)
    assert host(model.cluster_centers_).dtype == dtype
    assert host(model.labels_).shape == ((B, N) if batched else (N,))
    for b in range(B):
        check_fit(one_problem(model, b, batched), refs[b], f'{SHAPES[i][:4]} b={b}')
    # the seeding, fed the restatement's draws
    xd = _torch().from_numpy(x).cuda()
    randoms = np.stack([s[0] for s in seeds])
    indices, centers = km()._call_plusplus(xd, K, None, randoms, ok.n_local_trials(K))
    for b in range(B):
        assert seeds[b][1]['gap'] > CONDITION, seeds[b][1]['gap']
        np.testing.assert_array_equal(host(indices)[b], seeds[b][1]['indices'])
        np.testing.assert_array_equal(host(centers)[b], seeds[b][1]['centers'])
    # prediction from the fitted centres reproduces the labels, one-hot in the dtype of x
    hot = km().BinaryGMM(kmeans=model).predict(xin)
    assert hot.dtype == dtype and hot.shape == ((B, K, N) if batched else (K, N))
    np.testing.assert_array_equal(hot.argmax(axis=-2), host(model.labels_))
    np.testing.assert_array_equal(hot.sum(axis=-2), np.ones_like(hot.sum(axis=-2)))


# ---- the recorded cases: every way to stop, empty clusters --------------------------------------
@functools.lru_cache(maxsize=None)
def lloyd_reference(name):
    case = next(c for c in ok.LLOYD_CASES if c[0] == name)
    x, init = ok.lloyd_case(case)
    return case, x, init, ok.lloyd(x, init, max_iter=case[6], tol=case[5])


STOPS = {'blobs_5000_40_3': 'strict', 'blobs_4099_20_8': 'tol', 'blobs_4099_20_8_tol0': 'strict',
         'max_iter_3': 'max_iter', 'one_empty': 'tol', 'two_empty': 'strict',
         'two_empty_one_iter': 'max_iter', 'line_1000_1_2': 'strict'}


@pytest.mark.parametrize('name', sorted(STOPS))
def test_stopping_rules_and_empty_clusters(name):
    case, x, init, ref = lloyd_reference(name)
    assert ref['stop'] == STOPS[name], ref['stop']
    model = km().KMeans(n_clusters=case[3], init=init, max_iter=case[6], tol=case[5]).fit(x)
    check_fit(model, ref, name)
    # labels consistent with the final centres, however the loop ended
    np.testing.assert_array_equal(model.predict(x), model.labels_)
    assert isinstance(model.inertia_, float) and isinstance(model.n_iter_, int)


def test_two_empty_clusters_with_duplicated_rows():
    """Every row twice: the two farthest rows are a pair at the same distance, the lower index
    goes to the first empty class."""
    case, x, init, _ = lloyd_reference('two_empty')
    x2 = np.concatenate([x, x])
    ref = ok.lloyd(x2, init, max_iter=1)
    first = ok.sq_dist(x2, init).min(axis=1)  # distance to the own centre at the first labelling
    far = np.argsort(-first, kind='stable')[:2]
    assert far[1] == far[0] + len(x)
    model = km().KMeans(n_clusters=case[3], init=init, max_iter=1).fit(x2)
    assert ref['margin'] == 0.0  # both relocated centres are the same point
    check_fit(model, ref, 'duplicated rows', exact_ties=True)


def test_duplicate_centres_give_the_lowest_index():
    x = ok.make_data(1000, 5, 3, 31).astype(np.float32)
    centers = ok.initial_centers(x.astype(np.float64), 3, 31)
    centers[1] = centers[0]

    class Fitted:
        cluster_centers_ = centers
        n_clusters = 3

    hot = km().BinaryGMM(kmeans=Fitted()).predict(x)
    assert hot.dtype == np.float32 and hot.shape == (3, 1000)
    want = np.argmin(ok.sq_dist(x.astype(np.float64), centers), axis=1)
    assert not (want == 1).any() and (want == 0).any()
    np.testing.assert_array_equal(hot.argmax(axis=0), want)
    np.testing.assert_array_equal(hot[1], 0)


# ---- saliency ----------------------------------------------------------------------------------
def test_saliency_equals_fit_on_selected_rows():
    x = ok.make_data(3001, 12, 4, 41)
    sel = np.random.RandomState(1).rand(3001) < 0.55
    init = ok.initial_centers(x[sel], 4, 41)
    ref = ok.lloyd(x[sel], init)
    masked = km().KMeans(n_clusters=4, init=init).fit(x, sel)
    plain = km().KMeans(n_clusters=4, init=init).fit(x[sel])
    check_fit(plain, ref, 'selected rows')
    assert masked.n_iter_ == ref['n_iter']
    np.testing.assert_array_equal(masked.labels_[sel], ref['labels'])
    check_centers(masked.cluster_centers_, ref['centers'], 'saliency')
    assert abs(masked.inertia_ / ref['inertia'] - 1) <= TOL
    # the trainer, seeding included
    from pb_bss_amd.distribution import BinaryGMMTrainer
    a = BinaryGMMTrainer().fit(x, 4, saliency=sel, random_state=4)
    b = BinaryGMMTrainer().fit(x[sel], 4, random_state=4)
    rnd = ok.draw_randoms(np.random.RandomState(4), 4)
    seed = ok.kmeans_plusplus(x[sel], 4, rnd)
    assert seed['gap'] > CONDITION
    check_fit(b.kmeans, ok.lloyd(x[sel], seed['centers']), 'trainer on selected rows')
    check_centers(a.kmeans.cluster_centers_, b.kmeans.cluster_centers_, 'trainer with saliency')
    np.testing.assert_array_equal(a.predict(x)[:, sel], b.predict(x[sel]))


def test_too_few_rows_raise_value_error():
    from pb_bss_amd.distribution import BinaryGMMTrainer
    x = ok.make_data(50, 3, 2, 51)
    with pytest.raises(ValueError):
        BinaryGMMTrainer().fit(x[:3], 4)
    sel = np.zeros(50, bool)
    sel[:3] = True
    with pytest.raises(ValueError):
        BinaryGMMTrainer().fit(x, 4, saliency=sel)
    t = _torch()
    with pytest.raises(ValueError):  # the count is taken on the device
        km().KMeans(n_clusters=4, init=x[:4]).fit(t.from_numpy(x).cuda(), t.from_numpy(sel).cuda())
    BinaryGMMTrainer().fit(x, 3, saliency=sel)  # K == selected rows is served


# ---- determinism -------------------------------------------------------------------------------
def attributes(model):
    return [host(getattr(model, n)) for n in ('cluster_centers_', 'labels_', 'inertia_', 'n_iter_')]


def test_block_length_and_repeat_are_bit_identical():
    case, x, init, ref = lloyd_reference('blobs_4099_20_8')
    assert ref['n_iter'] > km().DEFAULT_BLOCK  # the stop falls behind the first block
    make = lambda: km().KMeans(n_clusters=case[3], init=init, tol=case[5])  # noqa: E731
    default = attributes(make().fit(x))
    for other in (make().fit(x, block=1), make().fit(x), make().fit(x, block=5)):
        for a, b in zip(default, attributes(other)):
            np.testing.assert_array_equal(a, b)
    x3 = np.stack([x, x[::-1], x])  # a batch stops problem by problem
    batch = make().fit(x3)
    single = make().fit(x3, block=1)
    for a, b in zip(attributes(batch), attributes(single)):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(default, attributes(batch)):
        np.testing.assert_array_equal(a, b[0])


def test_n_init_picks_the_lowest_inertia():
    x = ok.make_data(1200, 2, 6, 61)
    model = km().KMeans(n_clusters=6, init='random', n_init=5, random_state=3).fit(x)
    rs = np.random.RandomState(3)
    runs = []
    for _ in range(5):
        runs.append(ok.lloyd(x, x[rs.choice(1200, 6, replace=False)]))
        assert runs[-1]['margin'] > CONDITION
    inertias = [r['inertia'] for r in runs]
    best = runs[int(np.argmin(inertias))]
    assert max(inertias) > min(inertias) * (1 + 1e-6)  # the choice matters
    check_fit(model, best, 'n_init=5')
    assert km().KMeans(3, init='random')._runs() == 10 and km().KMeans(3)._runs() == 1


def test_default_trainer_follows_numpy_seed():
    from pb_bss_amd.distribution import BinaryGMM, BinaryGMMTrainer
    x = ok.make_data(2500, 12, 5, 71).astype(np.float32)
    np.random.seed(9)
    a = BinaryGMMTrainer().fit(x, 5)
    np.random.seed(9)
    b = BinaryGMMTrainer().fit(x, 5)
    assert isinstance(a, BinaryGMM)
    for u, v in zip(attributes(a.kmeans), attributes(b.kmeans)):
        np.testing.assert_array_equal(u, v)
    np.random.seed(9)
    wide = x.astype(np.float64)
    seed = ok.kmeans_plusplus(wide, 5, ok.draw_randoms(np.random.mtrand._rand, 5))
    assert seed['gap'] > CONDITION
    check_fit(a.kmeans, ok.lloyd(wide, seed['centers']), 'default trainer')
    hot = a.predict(x)
    assert hot.shape == (5, 2500) and hot.dtype == np.float32
    np.testing.assert_array_equal(hot.argmax(axis=0), a.kmeans.labels_)


def test_tensor_in_tensor_out():
    from pb_bss_amd.distribution import BinaryGMMTrainer
    t = _torch()
    x = ok.make_data(700, 6, 3, 81).astype(np.float32)
    init = ok.initial_centers(x.astype(np.float64), 3, 81)
    xd = t.from_numpy(np.stack([x, x[::-1].copy()])).cuda()
    model = BinaryGMMTrainer().fit(xd, 3, initialization=t.from_numpy(init).cuda())
    k = model.kmeans
    for a, dtype, shape in ((k.cluster_centers_, t.float32, (2, 3, 6)), (k.labels_, t.int32, (2, 700)),
                            (k.inertia_, t.float64, (2,)), (k.n_iter_, t.int32, (2,))):
        assert t.is_tensor(a) and a.is_cuda and a.dtype == dtype and tuple(a.shape) == shape
    hot = model.predict(xd)
    assert t.is_tensor(hot) and hot.is_cuda and hot.dtype == t.float32
    assert tuple(hot.shape) == (2, 3, 700)
    ref = ok.lloyd(x.astype(np.float64), init)
    check_fit(one_problem(k, 0, True), ref, 'tensor input')
    np.testing.assert_array_equal(host(hot[0]).argmax(axis=0), ref['labels'])
    hot64 = model.predict(xd.double())
    assert hot64.dtype == t.float64


def test_full_size_embedding():
    """The embedding of BASELINE configs[4]: five iterations from given centres."""
    N, E, K = 256500, 40, 3
    x = ok.make_data(N, E, K, 91).astype(np.float32)
    wide = x.astype(np.float64)
    init = ok.initial_centers(wide, K, 91)
    ref = ok.lloyd(wide, init, max_iter=5, tol=0.0)
    model = km().KMeans(n_clusters=K, init=init, max_iter=5, tol=0.0).fit(x)
    check_fit(model, ref, 'full size')
