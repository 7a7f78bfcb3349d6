"""GPU: the result of a call does not depend on what the same handle ran before it.

Every entry point that takes memory from the handle -- the grow-only `work` and `scratch` slabs,
the exchange buffer `cfg.xbuf` of the split groups / the cooperative launches / the joint
finalize, the `team_buf` of the DHTV teams -- carves its pieces from offset 0 of memory that the
previous call left as it was.  The family tests compare each kernel with its float64 oracle on a
handle whose history is whatever the fixed order of the suite made it; here the history is the
variable.  For every row of FAMILIES the result R0 of the FIRST call of a fresh handle is compared
with the family's oracle (at the tolerance of the family's own test file, cited per row), and the
same call is then repeated on one further fresh handle behind each of these predecessors:

  P1  the same call on other data (every carved piece holds plausible values of another problem),
  P2  the same call at a shape larger in every dimension (every piece at another offset),
  P3  one call of every other row of the table (every other user of the slabs and of xbuf); for
      the families that keep words in xbuf additionally every ordered pair of them,
  P4  the same call on an input with one non-finite entry, not checked,
  P5  calls the library refuses (argument sets of tests/test_gpu_capi_errors.py),
  P6  (split and team rows) a time-out of the inter-workgroup protocol that the engine consumed.

Two calls on one input on one handle are bit-identical for every row (asserted per row: the
precondition), so every result must equal R0 bit for bit -- floating outputs, mappings, status
words and iteration counts alike; no tolerance is involved.  NOT_REPRODUCIBLE names the rows for
which the precondition is known not to hold, with the measured call-to-call difference; those are
compared with the oracle at the family's tolerance instead.  pbbss_split_error is 0 after every
sequence.

tests/test_call_order_table.py keeps the table complete: every export of _lib.SIGNATURES is a key
of FAMILIES or a member of NO_HANDLE_MEMORY.
"""
import contextlib
import ctypes
import functools
import threading
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- plumbing ------------------------------------------------------------------------------------
def _dev(x, dtype=None):
    from pb_bss_amd import _lib
    return _lib.to_device(x, dtype)


def _host(x):
    if x is None or isinstance(x, np.ndarray):
        return x
    if hasattr(x, 'detach'):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@contextlib.contextmanager
def fresh_handle():
    """Inside the block `_lib.handle()` of this thread is a NEW handle (its slabs not allocated
    yet, its control buffers as pbbss_create left them); on exit the device is drained, the new
    handle destroyed and the thread's previous handle put back, with the settings the engine
    remembers for it.  While the block is active the device has two live handles, so the residency
    gate between handles is armed: that changes how long gated launches wait, not what they
    compute.  (A new host thread would not do: handles are keyed by threading.get_ident(), idents
    are recycled, and a "new" thread can inherit a used handle.)"""
    from pb_bss_amd import _lib, engine
    torch = _lib.require_gpu()
    key = (torch.cuda.current_device(), threading.get_ident())
    torch.cuda.synchronize()
    with _lib._handles_lock:
        old = _lib._handles.pop(key, None)
    old_settings = engine._SETTINGS.pop(key, None)
    try:
        yield _lib.handle(key[0])
    finally:
        torch.cuda.synchronize()
        with _lib._handles_lock:
            new = _lib._handles.pop(key, None)
            if old is not None:
                _lib._handles[key] = old
        engine._SETTINGS.pop(key, None)
        if old_settings is not None:
            engine._SETTINGS[key] = old_settings
        if new is not None:
            _lib.check(_lib.load().pbbss_destroy(new), 'pbbss_destroy')


def _cu_count():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _status_errors():
    from pb_bss_amd import _lib, engine
    return (engine.StatusAssertionError, engine.StatusLinAlgError, _lib.PbbssError, ValueError,
            FloatingPointError, np.linalg.LinAlgError)


class Row:
    """One row of the table.

    exports   the C entry points the Python call reaches that take memory from the handle
    call      the Python call, for the record
    shape     variant -> shape tuple: 'small' (the smallest shape that reaches the handle's memory
              on this path, from the family's own test file) and 'big' (larger in every dimension
              the path allows)
    make      (shape, seed) -> inputs (host arrays, read-only; built once)
    run       (inputs, checked) -> {name: host array}; checked=False: no status check where the
              call has such a switch
    oracle    (inputs, outputs) -> None; asserts against the float64 oracle
    poison    inputs -> inputs with one non-finite entry
    xbuf      the name of the xbuf convention the row uses, or None
    timeout   a callable () that runs the family through the checked public entry point (the
              one that consumes a time-out), for P6; None for rows without bounded waits"""

    def __init__(self, exports, call, shape, make, run, oracle, poison, seeds=(0, 1), xbuf=None,
                 timeout=None, cite=''):
        self.exports, self.call, self.shape, self.make_fn = tuple(exports), call, shape, make
        self.run, self.oracle, self.poison, self.seeds = run, oracle, poison, seeds
        self.xbuf, self.timeout, self.cite = xbuf, timeout, cite

    def inputs(self, variant='small', which=0):
        shape = self.shape[variant]
        shape = shape() if callable(shape) else shape
        return _inputs(self, shape, self.seeds[which])


@functools.lru_cache(maxsize=None)
def _inputs(row, shape, seed):
    inp = row.make_fn(shape, seed)
    _frozen(*inp.values())
    return inp


def _nan_at(inp, key, index):
    out = dict(inp)
    a = np.array(inp[key])
    a[index] = np.nan
    out[key] = a
    return out


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _largest_difference(got, want):
    worst = {}
    for name in want:
        a, b = got[name], want[name]
        if a is None or b is None:
            assert a is b, name
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        if _bits(a) != _bits(b):
            both = np.isfinite(a.astype(np.complex128)) & np.isfinite(b.astype(np.complex128))
            diff = np.abs(a.astype(np.complex128)[both] - b.astype(np.complex128)[both])
            worst[name] = (float(diff.max()) if diff.size else 0.0, int((~both).sum()))
    return worst


# ---- the families ----------------------------------------------------------------------------------
def _make_stft(shape, seed):
    from pb_bss_amd.testing import synth
    F, T, D, K = shape
    Y, init = synth.make_stft(F, T, D, K, seed=seed)
    return dict(Y=Y, init=init)


def _em_outputs(r):
    return {k: _host(v) for k, v in r.items()}


def _em_fit(iterations, **kw):
    def run(inp, checked=True):
        from pb_bss_amd import engine
        K = inp['init'].shape[-2]
        r = engine.em_fit(_dev(inp['Y']), K, gamma0=_dev(inp['init']), iterations=iterations,
                          final_predict=True, check_status=checked, **kw)
        return _em_outputs(r)
    return run


def _em_oracle(iterations, mask_tol=1e-7, weight_tol=1e-8, tight_bins=None, tight_tol=None, **kw):
    """tests/test_gpu_wave_roles.py::_check (trajectories of 2 .. 20 iterations: mask 1e-7, weight
    1e-8) on EVERY bin; `tight_bins`: the bins the family test holds to `tight_tol` on top
    (::test_member_workgroups_of_the_remainder_bin: the last two to 1e-9).  The packed-FP32 rows
    pass the bounds of tests/test_gpu_f32.py (5e-4 on the masks, no bound on the weight)."""
    def check(inp, out):
        from oracle import cacgmm as oc
        Y128 = inp['Y'].astype(np.complex128)
        m = oc.em_fit(Y128, inp['init'], iterations=iterations, **kw)
        mask = oc.em_predict(m, Y128)
        assert (out['status'] & 3 == 0).all(), out['status']
        err = np.abs(out['affiliation'] - mask).max()
        print(f'R0 against the oracle: mask {err:.3e}')
        assert err < mask_tol, err
        if weight_tol is not None:
            werr = np.abs(out['weight'][..., None] - m['weight']).max()
            assert werr < weight_tol, werr
        if tight_bins is not None:
            sel = tight_bins(inp['Y'].shape[0])
            assert np.abs(out['affiliation'][sel] - mask[sel]).max() < tight_tol
    return check


def _poison_frames(inp):
    return _nan_at(inp, 'Y', (0, 5, 0))


def _split_shape():
    return (_cu_count() + 1, 128, 2, 3)     # tests/test_gpu_wave_roles.py::_split_problem


def _split_big():
    return (_cu_count() + 2, 200, 3, 4)


# ---- P6: predecessors that MUST time out with one poll per bounded wait: the shapes and the
# warnings of tests/test_gpu_timeouts.py (257 bins: one bin more than compute units, long rows)
@functools.lru_cache(maxsize=None)
def _timeout_stft(F, T, D, K, seed):
    from pb_bss_amd.testing import synth
    return _frozen(*synth.make_stft(F, T, D, K, seed=seed))


def _split_timeout():
    """::test_split_groups_really_time_out_and_the_fit_is_repeated"""
    from pb_bss_amd import engine
    Y, init = _timeout_stft(257, 512, 4, 2, 31)
    engine.em_fit(_dev(Y), 2, gamma0=_dev(init), iterations=8, final_predict=True)


_split_timeout.match = 'split groups'


def _shared_run(inp, checked=True):
    from pb_bss_amd import _lib, engine
    F, K = inp['Y'].shape[0], inp['init'].shape[-2]
    r = engine.em_fit_shared(_dev(inp['Y']), K, F, weight_mode=_lib.WEIGHT_SHARED_K,
                             gamma0=_dev(inp['init']), iterations=6, final_predict=True,
                             check_status=checked)
    assert r is not None, 'the cooperative kernel serves a few small bins'
    return _em_outputs(r)


def _shared_oracle(inp, out):
    """tests/test_gpu_wave_roles.py::test_shared_weight_kernel: mask 1e-7, weight 1e-8"""
    from oracle import cacgmm as oc
    K = inp['init'].shape[-2]
    Y128 = inp['Y'].astype(np.complex128)
    m = oc.em_fit(Y128, inp['init'], iterations=6, weight_constant_axis=(-3, -1))
    assert (out['status'] & 3 == 0).all()
    assert np.abs(out['affiliation'] - oc.em_predict(m, Y128)).max() < 1e-7
    assert np.abs(out['weight'].reshape(K) - np.asarray(m['weight']).reshape(K)).max() < 1e-8


def _shared_timeout():
    """::test_cooperative_shared_weight_launch_really_times_out"""
    from pb_bss_amd.distribution import CACGMMTrainer
    Y, init = _timeout_stft(257, 700, 8, 3, 33)
    CACGMMTrainer().fit_predict(Y, initialization=init, iterations=5,
                                weight_constant_axis=(-3, -1))


_shared_timeout.match = 'cooperative shared-weight launch timed out'


def _generic_parts_run(inp, checked=True):
    """one M step and one E step of the generic-size path on their own exports"""
    from pb_bss_amd import _lib, engine
    y = _dev(inp['Y'])
    vec, val, _, st = engine.cacg_m_step(y, _dev(inp['init']), _dev(np.ones_like(inp['init'])),
                                         layout=_lib.LAYOUT_TD, check_status=checked)
    aff, _, _ = engine.em_predict(y, vec, val, _dev(inp['weight']))
    return dict(eigval=_host(val), status=_host(st), affiliation=_host(aff))


def _generic_parts_make(shape, seed):
    inp = _make_stft(shape, seed)
    inp['weight'] = np.ascontiguousarray(inp['init'].mean(-1))
    return inp


def _generic_parts_oracle(inp, out):
    """tests/test_gpu_generic.py: a single step to 1e-9.  The first iteration of the oracle's loop
    is this M step (affiliations = the initialisation, quadratic form = ones)."""
    from oracle import cacgmm as oc
    Y128 = inp['Y'].astype(np.complex128)
    m = oc.em_fit(Y128, inp['init'], iterations=1)
    assert (out['status'] & 3 == 0).all()
    assert np.abs(out['eigval'] - m['eigval']).max() < 1e-9
    m = dict(m, weight=inp['weight'][..., None])
    assert np.abs(out['affiliation'] - oc.em_predict(m, Y128)).max() < 1e-9


def _psd_make(shape, seed):
    F, T, D, K = shape
    inp = _make_stft(shape, seed)
    inp['X'] = np.ascontiguousarray(inp['Y'].transpose(0, 2, 1))
    return inp


def _psd_run(inp, checked=True):
    from pb_bss_amd import engine
    return dict(psd=_host(engine.psd(_dev(inp['X']), _dev(inp['init']))))


def _psd_oracle(inp, out):
    """tests/test_gpu_cwmm.py / tests/test_gpu_generic.py: the masked PSD to 1e-11"""
    from oracle import beamformer as ob
    want = ob.psd(inp['X'].astype(np.complex128), inp['init'])
    assert np.abs(out['psd'] - want).max() < 1e-11


def _trainer_masks(make_trainer, iterations, **kw):
    def run(inp, checked=True):
        trainer = make_trainer()
        extra = {k: inp[k] for k in ('saliency',) if k in inp}
        args = (inp['Y'], inp['e']) if 'e' in inp else (inp['Y'],)
        masks = trainer.fit_predict(*args, initialization=inp['init'], iterations=iterations,
                                    **extra, **kw)
        return dict(masks=_host(masks))
    return run


def _cwmm():
    from pb_bss_amd.distribution import CWMMTrainer
    return CWMMTrainer()


def _cwmm_oracle(inp, out):
    """tests/test_gpu_cwmm.py: masks after a few iterations to 1e-7, on every bin (also
    ::test_cwmm_remainder_bins_as_split_groups, for the row with a remainder bin)"""
    from oracle import cwmm as ow
    Y128 = inp['Y'].astype(np.complex128)
    ref = ow.cwmm_predict(ow.cwmm_fit(Y128, inp['init'], iterations=6), Y128)
    assert np.abs(out['masks'] - ref).max() < 1e-7


def _last_bins(F):
    return [F - 2, F - 1]


def _cwmm_timeout():
    """::test_watson_split_groups_really_time_out"""
    Y, init = _timeout_stft(257, 512, 4, 2, 32)
    _cwmm().fit_predict(Y, initialization=init, iterations=6)


_cwmm_timeout.match = 'split groups'


def _cbmm_make(shape, seed):
    """tests/test_gpu_cbmm.py::mixture"""
    F, T, D, K = shape
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((F, T, D)) + 1j * rng.standard_normal((F, T, D)))
    dirs = rng.standard_normal((F, K, D)) + 1j * rng.standard_normal((F, K, D))
    lab = rng.integers(0, K, size=(F, T))
    y += 3 * np.take_along_axis(dirs, lab[..., None], axis=1) * rng.standard_normal((F, T, 1))
    init = rng.uniform(size=(F, K, T))
    init /= init.sum(1, keepdims=True)
    return dict(Y=y, init=init)


def _cbmm_run(inp, checked=True):
    from pb_bss_amd.distribution import CBMMTrainer
    model = CBMMTrainer().fit(inp['Y'], initialization=inp['init'], iterations=20)
    return dict(weight=_host(np.asarray(model.weight)), masks=_host(model.predict(inp['Y'])))


def _cbmm_oracle(inp, out):
    """tests/test_gpu_cbmm.py::test_trainer_vs_oracle: weight 1e-9, masks 1e-8"""
    import oracle_cbmm as oc
    ref = oc.cbmm_fit(inp['Y'], inp['init'], 20)
    assert np.abs(out['weight'] - ref['weight']).max() < 1e-9
    assert np.abs(out['masks'] - oc.cbmm_predict(ref, inp['Y'])).max() < 1e-8


def _joint_make(shape, seed):
    from oracle import synth
    F, T, D, K, E = shape
    Y, e, init = synth.make_joint(F, T, D, K, E, seed=seed)
    return dict(Y=Y, e=e, init=init)


def _joint_trainer(kind):
    def make():
        from pb_bss_amd.distribution import GCACGMMTrainer, VMFCACGMMTrainer
        return GCACGMMTrainer() if kind == 'gaussian' else VMFCACGMMTrainer()
    return make


def _joint_oracle(kind, **kw):
    """tests/test_gpu_embed.py::test_joint_models_every_sensor_count_translation_unit: 1e-6"""
    def check(inp, out):
        from oracle import embed as oe
        Y128, e64 = inp['Y'].astype(np.complex128), inp['e'].astype(np.float64)
        ref = oe.joint_fit(kind, Y128, e64, inp['init'], 4, **kw)
        assert np.abs(out['masks'] - oe.joint_model_predict(ref, Y128, e64)).max() < 1e-6
    return check


def _mixture_make(spread, noise):
    """tests/test_gpu_embed_wide.py::_mixture_data"""
    def make(shape, seed):
        N, E, K = shape
        rng = np.random.default_rng(seed)
        mu = rng.standard_normal((K, E)) * spread
        lab = rng.integers(K, size=(N,))
        y = np.take_along_axis(mu, lab[..., None], -2) + noise * rng.standard_normal((N, E))
        init = rng.uniform(size=(K, N)) + 2.0 * (np.arange(K)[:, None] == lab[..., None, :])
        init /= init.sum(-2, keepdims=True)
        return dict(Y=y.astype(np.float32), init=init, saliency=rng.uniform(0.1, 1.0, size=(N,)))
    return make


def _vmfmm_run(inp, checked=True):
    from pb_bss_amd.distribution import VMFMMTrainer
    model = VMFMMTrainer().fit(inp['Y'], initialization=inp['init'], iterations=6,
                               saliency=inp['saliency'])
    return dict(mean=_host(model.vmf.mean), concentration=_host(model.vmf.concentration),
                weight=_host(model.weight), masks=_host(model.predict(inp['Y'])))


def _vmfmm_oracle(inp, out):
    """tests/test_gpu_embed.py::test_vmfmm_shapes_against_oracle and
    tests/test_gpu_embed_wide.py::test_vmfmm_wide_shapes_against_oracle"""
    from oracle import embed as oe
    y64 = inp['Y'].astype(np.float64)
    ref = oe.vmfmm_fit(y64, inp['init'], 6, saliency=inp['saliency'])
    np.testing.assert_allclose(out['mean'], ref['mean'], atol=1e-9)
    np.testing.assert_allclose(out['concentration'], ref['concentration'], rtol=1e-8)
    np.testing.assert_allclose(out['weight'], ref['weight'], atol=1e-10)
    np.testing.assert_allclose(out['masks'], oe.vmfmm_predict(ref, y64), atol=1e-8)


def _gmm_run(inp, checked=True):
    from pb_bss_amd.distribution import GMMTrainer
    m = GMMTrainer().fit(inp['Y'], initialization=inp['init'], iterations=6,
                         saliency=inp['saliency'], covariance_type='spherical')
    return dict(mean=_host(m.gaussian.mean), covariance=_host(m.gaussian.covariance),
                weight=_host(m.weight), masks=_host(m.predict(inp['Y'])))


def _gmm_oracle(inp, out):
    """tests/test_gpu_embed.py::test_gmm_shapes_against_oracle and
    tests/test_gpu_embed_wide.py::test_gmm_spherical_wide_shapes_against_oracle"""
    from oracle import embed as oe
    y64 = inp['Y'].astype(np.float64)
    o = oe.gmm_fit(y64, inp['init'], 6, saliency=inp['saliency'])
    np.testing.assert_allclose(out['mean'], o['mean'], atol=1e-9)
    np.testing.assert_allclose(out['covariance'], o['covariance'], rtol=1e-9)
    np.testing.assert_allclose(out['weight'], o['weight'], atol=1e-10)
    np.testing.assert_allclose(out['masks'], oe.gmm_predict(o, y64), atol=1e-7)


def _gmm_full_run(inp, checked=True):
    from pb_bss_amd.distribution import GMMTrainer
    m = GMMTrainer().fit(inp['Y'], initialization=inp['init'], iterations=5)
    return dict(mean=_host(m.gaussian.mean), covariance=_host(m.gaussian.covariance),
                weight=_host(m.weight), masks=_host(m.predict(inp['Y'])))


def _gmm_full_oracle(inp, out):
    """tests/test_gpu_embed.py::test_gmm_full_covariance_matches_reference_and_oracle"""
    from oracle import embed as oe
    y64 = inp['Y'].astype(np.float64)
    o = oe.gmm_fit(y64, inp['init'], 5, covariance_type='full')
    np.testing.assert_allclose(out['mean'], o['mean'], atol=1e-8)
    np.testing.assert_allclose(out['covariance'], o['covariance'], atol=1e-8)
    np.testing.assert_allclose(out['weight'], o['weight'], atol=1e-9)
    np.testing.assert_allclose(out['masks'], oe.gmm_predict(o, y64, 'full'), atol=1e-6)


def _single_make(shape, seed):
    """tests/test_gpu_embed.py::test_gaussian_full_covariance_against_oracle"""
    N, E, K = shape
    rng = np.random.default_rng(seed)
    A = 0.6 * np.eye(E) + 0.4 * rng.normal(size=(E, E)) / np.sqrt(E)
    y = (rng.normal(size=(N, E)) @ A + rng.normal(size=E) * 3).astype(np.float32)
    return dict(Y=y, saliency=rng.uniform(size=(K, N)) ** 2)


def _single_run(covariance_type):
    def run(inp, checked=True):
        from pb_bss_amd.distribution import GaussianTrainer
        m = GaussianTrainer().fit(inp['Y'][None], saliency=inp['saliency'],
                                  covariance_type=covariance_type)
        return dict(mean=_host(m.mean), covariance=_host(m.covariance),
                    log_pdf=_host(m.log_pdf(inp['Y'][None])))
    return run


def _single_oracle(covariance_type):
    """tests/test_gpu_embed.py::test_gaussian_full_covariance_against_oracle (mean 1e-11,
    covariance 1e-11 of its largest entry, log-pdf rtol 1e-9 atol 1e-7), also for the spherical
    fit, whose sums are the trace of the same scatter"""
    def check(inp, out):
        from oracle import embed as oe
        y64 = inp['Y'].astype(np.float64)
        om, oc = oe.gaussian_fit(y64[None], inp['saliency'], covariance_type)
        np.testing.assert_allclose(out['mean'], om, atol=1e-11)
        np.testing.assert_allclose(out['covariance'], oc, atol=1e-11 * np.abs(oc).max())
        ref = oe.gaussian_log_pdf(y64[None], om, oc, covariance_type)
        np.testing.assert_allclose(out['log_pdf'], ref, rtol=1e-9, atol=1e-7)
    return check


def _mixw_make(shape, seed):
    Bo, Bi, K, N = shape
    rng = np.random.default_rng(seed)
    aff = rng.uniform(size=shape)
    aff /= aff.sum(-2, keepdims=True)
    return dict(Y=aff, saliency=rng.uniform(size=(Bo, Bi, N)))


def _mixw_run(inp, checked=True):
    from pb_bss_amd import engine
    out = engine.estimate_mixture_weight(_dev(inp['Y']), _dev(inp['saliency']), True, True)
    return dict(weight=_host(out))


def _mixw_oracle(inp, out):
    """tests/test_gpu_api.py::test_estimate_mixture_weight_kernel_against_numpy: 1e-13"""
    from pb_bss_amd.distribution.mixture_model_utils import estimate_mixture_weight
    want = estimate_mixture_weight(inp['Y'], inp['saliency'], (-3, -1))
    assert np.abs(out['weight'] - want).max() < 1e-13


def _kmeans_make(shape, seed):
    import oracle_kmeans as ok
    N, E, K = shape
    x = ok.make_data(N, E, K, 100 + seed)
    return dict(Y=x, init=ok.initial_centers(x, K, 100 + seed),
                randoms=ok.draw_randoms(np.random.RandomState(200 + seed), K))


def _kmeans_run(inp, checked=True):
    import oracle_kmeans as ok
    import torch
    from pb_bss_amd.distribution import kmeans
    K = inp['init'].shape[0]
    model = kmeans.KMeans(n_clusters=K, init=inp['init'], max_iter=300).fit(inp['Y'])
    hot = kmeans.BinaryGMM(kmeans=model).predict(inp['Y'])
    xd = torch.from_numpy(np.array(inp['Y'][None])).cuda()
    indices, centers = kmeans._call_plusplus(xd, K, None, inp['randoms'][None],
                                             ok.n_local_trials(K))
    return dict(labels=_host(model.labels_), centers=_host(model.cluster_centers_),
                inertia=np.asarray(_host(model.inertia_)), n_iter=np.asarray(_host(model.n_iter_)),
                one_hot=_host(hot), seed_indices=_host(indices), seed_centers=_host(centers))


def _kmeans_oracle(inp, out):
    """tests/test_gpu_kmeans.py::check_fit / test_shapes_fit_and_seeding: discrete results exact
    under the margin / gap conditions, centres 1e-10, inertia 1e-10 relative"""
    import oracle_kmeans as ok
    K = inp['init'].shape[0]
    ref = ok.lloyd(inp['Y'], inp['init'], max_iter=300)
    assert ref['margin'] > 1e-9
    assert int(out['n_iter']) == ref['n_iter']
    np.testing.assert_array_equal(out['labels'], ref['labels'])
    assert np.abs(out['centers'] - ref['centers']).max() <= 1e-10
    assert abs(float(out['inertia']) - ref['inertia']) <= 1e-10 * ref['inertia']
    np.testing.assert_array_equal(out['one_hot'].argmax(axis=-2), ref['labels'])
    seed = ok.kmeans_plusplus(inp['Y'], K, inp['randoms'])
    assert seed['gap'] > 1e-9
    np.testing.assert_array_equal(out['seed_indices'][0], seed['indices'])
    np.testing.assert_array_equal(out['seed_centers'][0], seed['centers'])


DHTV_PLAN = {(3, 33, 65): [[5, 0, 33], [2, 3, 20]], (4, 65, 130): [[5, 0, 65], [2, 3, 40]]}


def _dhtv_make(shape, seed):
    """tests/test_gpu_permutation_alignment.py::test_frame_slice_kernel_shapes_metrics_and_features"""
    K, F, T = shape
    rng = np.random.default_rng(K * 1000 + T + seed)
    U = 2
    act = rng.uniform(size=(U, K, 1, T)) ** 4
    mask = act * rng.uniform(0.3, 1.0, size=(U, K, F, T)) + 0.1 * rng.uniform(size=(U, K, F, T))
    for u in range(U):
        for f in range(F):
            mask[u, :, f] = mask[u, rng.permutation(K), f]
    return dict(Y=mask, plan=np.asarray(DHTV_PLAN[shape], np.int32))


def _dhtv_run(team):
    def run(inp, checked=True):
        from pb_bss_amd import engine
        try:
            engine.set_dhtv_team(team)
            mapping, feat, st = engine.dhtv_calculate_mapping(_dev(inp['Y']), _dev(inp['plan']))
            return dict(mapping=_host(mapping), features=_host(feat), status=_host(st))
        finally:
            engine.set_dhtv_team(0)
    return run


def _dhtv_oracle(inp, out):
    """tests/test_gpu_permutation_alignment.py (as above): mappings exact, the aligned unit-norm
    features to 1e-14"""
    from oracle import permutation_alignment as op
    mask, plan = inp['Y'], inp['plan'].tolist()
    F = mask.shape[2]
    assert (out['status'] == 0).all()
    for u in range(mask.shape[0]):
        want = op.dhtv_calculate_mapping(mask[u], plan, 'greedy', 'cos')
        assert np.array_equal(out['mapping'][u], want), u
        al = mask[u][want, range(F)]
        al = al / np.maximum(np.linalg.norm(al, axis=-1, keepdims=True), np.finfo(np.float64).tiny)
        assert np.abs(out['features'][u] - al).max() < 1e-14 * max(1.0, np.abs(al).max())


@functools.lru_cache(maxsize=None)
def _timeout_masks():
    """::test_dhtv_team_really_times_out"""
    rng = np.random.default_rng(34)
    K, F, T = 3, 257, 300
    act = rng.uniform(size=(K, 1, T)) ** 4
    mask = act * rng.uniform(0.5, 1.0, size=(K, F, T)) + 0.05 * rng.uniform(size=(K, F, T))
    mask /= mask.sum(0, keepdims=True)
    for f in range(F):
        mask[:, f] = mask[rng.permutation(K), f]
    return _frozen(mask)[0]


def _dhtv_timeout(team):
    def run():
        from pb_bss_amd import engine
        from pb_bss_amd.permutation_alignment import DHTVPermutationAlignment
        solver = DHTVPermutationAlignment.from_stft_size(512)
        try:
            engine.set_dhtv_team(team)
            solver.calculate_mapping(_timeout_masks())
        finally:
            engine.set_dhtv_team(0)
    run.match = 'co-resident'
    return run


ALIGNER = dict(segment_start=10, segment_width=20, segment_shift=5, main_iterations=8,
               sub_iterations=2)


def _aligner_run(inp, checked=True):
    from pb_bss_amd.distribution import CACGMMTrainer
    from pb_bss_amd.permutation_alignment import DHTVPermutationAlignment
    F = inp['Y'].shape[0]
    solver = DHTVPermutationAlignment(stft_size=2 * (F - 1), **ALIGNER)
    m = CACGMMTrainer().fit(inp['Y'], initialization=inp['init'], iterations=4,
                            weight_constant_axis=(-3,), inline_permutation_aligner=solver)
    return dict(weight=_host(np.asarray(m.weight)), masks=_host(m.predict(inp['Y'])))


def _aligner_oracle(inp, out):
    """tests/test_gpu_api.py::test_stepwise_fit_with_device_inline_aligner_matches_oracle (weight
    1e-9, masks 1e-7) with its reference loop, tests/test_gpu_api.py::_oracle_stepwise"""
    from oracle import cacgmm as oc, permutation_alignment as op
    from pb_bss_amd.permutation_alignment import DHTVPermutationAlignment
    F = inp['Y'].shape[0]
    plan = np.asarray(DHTVPermutationAlignment(stft_size=2 * (F - 1), **ALIGNER).alignment_plan)
    Y128 = inp['Y'].astype(np.complex128)
    yn = oc.normalize_observation(Y128)
    aff, q, model = inp['init'], np.ones_like(inp['init']), None
    for _ in range(4):
        if model is not None:
            aff, q, _ = oc.e_step(yn, model['weight'], model['eigvec'], model['eigval'],
                                  affiliation_eps=1e-10)
            kft = aff.transpose(1, 0, 2)
            mapping = op.dhtv_calculate_mapping(kft, plan)
            aff = op.apply_mapping(kft, mapping).transpose(1, 0, 2)
            q = op.apply_mapping(q.transpose(1, 0, 2), mapping).transpose(1, 0, 2)
        w, vec, lam = oc.m_step(yn, q, aff, saliency=None, weight_constant_axis=(-3,))
        model = dict(weight=w, eigvec=vec, eigval=lam)
    assert np.abs(out['weight'] - model['weight']).max() < 1e-9
    assert np.abs(out['masks'] - oc.em_predict(model, Y128)).max() < 1e-7


WPE_E_CASE = {(2, 3, 1, 64): 2.4e-13}   # tests/test_gpu_wpe.py::E_CASE, three iterations


def _wpe_make(shape, seed):
    import oracle_wpe as ow
    D, taps, delay, T = shape
    Y = ow.case_input(shape, np.complex128) if seed == 0 and shape in WPE_E_CASE else \
        ow.synth(ow.BATCH, D, T, seed=40 + seed)
    return dict(Y=Y, taps=taps, delay=delay)


def _wpe_run(inp, checked=True):
    from pb_bss_amd import transform
    return dict(X=_host(transform.wpe(inp['Y'], inp['taps'], inp['delay'], 3)))


def _wpe_oracle(inp, out):
    """tests/test_gpu_wpe.py::check_sweep: 16 max(E_CASE, 1e-13) relative to max |X|"""
    import oracle_wpe as ow
    shape = (inp['Y'].shape[1], inp['taps'], inp['delay'], inp['Y'].shape[2])
    want = ow.wpe(inp['Y'], inp['taps'], inp['delay'], 3, 0, 'full')
    err = np.abs(out['X'] - want).max() / np.abs(want).max()
    assert err <= 16 * max(WPE_E_CASE[shape], 1e-13), err


def _wpe_parts_run(inp, checked=True):
    from pb_bss_amd import transform
    inv = transform.get_power_inverse(inp['Y'])
    R, P = transform.get_correlations(inp['Y'], inv, inp['taps'], inp['delay'], 'full')
    return dict(inverse_power=_host(inv), R=_host(R), P=_host(P))


def _wpe_parts_oracle(inp, out):
    """tests/test_gpu_wpe.py::test_power_inverse (rtol 1e-13) and
    ::test_parts_and_their_composition (16 T eps of the largest entry)"""
    import oracle_wpe as ow
    T = inp['Y'].shape[2]
    np.testing.assert_allclose(out['inverse_power'], ow.power_inverse(inp['Y'], 0), rtol=1e-13)
    for b in range(inp['Y'].shape[0]):
        Rw, Pw = ow.correlations(inp['Y'][b], out['inverse_power'][b], inp['taps'], inp['delay'],
                                 'full')
        assert np.abs(out['R'][b] - Rw).max() <= 16 * T * 2.0 ** -52 * np.abs(Rw).max()
        assert np.abs(out['P'][b] - Pw).max() <= 16 * T * 2.0 ** -52 * np.abs(Pw).max()


def _istft_make(shape, seed):
    C, T, size, shift = shape
    rng = np.random.default_rng(size + shift + seed)
    F = size // 2 + 1
    return dict(Y=rng.standard_normal((C, T, F)) + 1j * rng.standard_normal((C, T, F)),
                size=size, shift=shift)


def _istft_run(inp, checked=True):
    from pb_bss_amd.transform import istft
    return dict(x=_host(istft(inp['Y'], inp['size'], inp['shift'], window='hann')))


def _istft_oracle(inp, out):
    """tests/test_gpu_stft.py::test_istft_matches_oracle: 1e-12"""
    from oracle import stft as o
    ref = o.istft(inp['Y'], inp['size'], inp['shift'], window='hann')
    np.testing.assert_allclose(out['x'], ref, atol=1e-12)


GRIFFIN_SEEDS = (11, 26)   # tests/oracle_griffin_lim.py::CASES 'size64' and 'batch_a'


def _griffin_make(shape, seed):
    import oracle_griffin_lim as og
    K, T, size, shift = shape
    c = og.gen_case(seed, K, T, size, shift)
    return dict(Y=c['X'], y=c['y'], size=size, shift=shift)


def _griffin_run(inp, checked=True):
    from pb_bss_amd import transform
    model = transform.MISI(inp['Y'], y=inp['y'], first_guess='y', size=inp['size'],
                           shift=inp['shift'], fading=False)
    model.step(iterations=5)
    return dict(x_hat=_host(model.x_hat), X_dash=_host(model.X_dash),
                X_dash_dash=_host(model.X_dash_dash))


def _griffin_oracle(inp, out):
    """tests/test_gpu_griffin_lim.py::check: (2 n + 1) 1e-11 after n iterations"""
    import oracle_griffin_lim as og
    ref = og.run(og.RESTATED['MISI'], inp['Y'], inp['y'], 'y', 5, size=inp['size'],
                 shift=inp['shift'], fading=False)
    bound = 11e-11
    assert np.abs(out['x_hat'] - ref.x_hat).max() < bound
    assert np.abs(out['X_dash'] - ref.X_dash).max() / np.abs(inp['Y']).max() < bound
    assert (np.abs(out['X_dash_dash'] - ref.X_dash_dash).max()
            / np.abs(ref.X_dash_dash).max()) < bound


def _si_sdr_make(shape, seed):
    import oracle_evaluation as oe
    r, e = oe.gen_si_sdr(shape[0] + shape[1] + seed, shape)
    return dict(Y=r, e=e)


def _si_sdr_run(inp, checked=True):
    from pb_bss_amd.evaluation import si_sdr
    from pb_bss_amd.evaluation.sxr_module import get_variance_for_zero_mean_signal
    return dict(si_sdr=_host(si_sdr(inp['Y'], inp['e'])),
                power=_host(get_variance_for_zero_mean_signal(inp['e'], axis=-1)))


def _si_sdr_oracle(inp, out):
    """tests/test_gpu_evaluation.py::check: 1e-9 dB; the power to 1e-13 relative (a mean of N
    squares in float64)"""
    import oracle_evaluation as oe
    assert np.abs(out['si_sdr'] - oe.si_sdr(inp['Y'], inp['e'])).max() <= 1e-9
    np.testing.assert_allclose(out['power'], oe.power(inp['e'], axis=-1), rtol=1e-13)


def _sxr_make(shape, seed):
    import oracle_evaluation as oe
    B, K, D, N = shape
    im, no = oe.gen_input_case(seed, (B,), K, D, N)
    co, cn = oe.gen_output_case(10 * K + K + seed, (B,), K, K, N)
    return dict(Y=im, noise=no, contribution=co, contribution_noise=cn)


def _sxr_run(inp, checked=True):
    from pb_bss_amd.evaluation.sxr_module import input_sxr, output_sxr
    got_in = input_sxr(inp['Y'], inp['noise'], True, True)
    got_out, sel = output_sxr(inp['contribution'], inp['contribution_noise'], True,
                              return_selection=True)
    out = {'in_' + name: _host(getattr(got_in, name)) for name in got_in._fields}
    out.update({'out_' + name: _host(getattr(got_out, name)) for name in got_out._fields})
    out['selection'] = _host(sel)
    return out


def _sxr_oracle(inp, out):
    """tests/test_gpu_evaluation.py::test_input_sxr / ::test_output_sxr: 1e-9 dB, the selection
    exact where its margin is at least oracle_evaluation.MARGIN"""
    import oracle_evaluation as oe
    want = oe.input_sxr(inp['Y'], inp['noise'], True, True)
    for name in want._fields:
        assert np.abs(out['in_' + name] - getattr(want, name)).max() <= 1e-9, name
    details = {}
    want, want_sel = oe.output_sxr(inp['contribution'], inp['contribution_noise'], True, details)
    assert details['margin'].min() >= oe.MARGIN
    np.testing.assert_array_equal(out['selection'], want_sel)
    for name in want._fields:
        assert np.abs(out['out_' + name] - getattr(want, name)).max() <= 1e-9, name


def _bss_make(shape, seed):
    import oracle_bss_eval as ob
    K, Ke, N, L = shape
    references, estimations = ob.gen_case(1000 * K + 100 * Ke + N + L + seed, K, Ke, N)
    return dict(Y=references, e=estimations, L=L)


def _bss_dependent_make(shape, seed):
    """tests/oracle_bss_eval.py::gen_dependent_case at any K: the last reference is the sum of the
    first two, a singular Gram matrix"""
    import oracle_bss_eval as ob
    K, Ke, N, L = shape
    references, estimations = ob.gen_case(7 + seed, K, Ke, N)
    references[K - 1] = references[0] + references[1]
    return dict(Y=references, e=estimations, L=L)


def _bss_run(inp, checked=True):
    from pb_bss_amd.evaluation import mir_eval_sources
    sdr, sir, sar, selection = mir_eval_sources(inp['Y'], inp['e'], filter_length=inp['L'])
    return dict(sdr=_host(sdr), sir=_host(sir), sar=_host(sar), selection=_host(selection))


def _bss_oracle(bound):
    """tests/test_gpu_bss_eval.py: BOUND = 1e-9 dB on the normal route (::test_parity),
    FALLBACK_BOUND = 1e-6 dB where the Gram matrix is singular and the host solves
    (::test_host_fallback_dependent_references)"""
    def check(inp, out):
        import oracle_bss_eval as ob
        expected = ob.bss_eval(inp['Y'], inp['e'], inp['L'], True, 'direct')
        assert out['selection'].tolist() == expected[3].tolist()
        for got, want in zip((out['sdr'], out['sir'], out['sar']), expected[:3]):
            assert ob.table_difference(got, want) < bound
    return check


def _stoi_make(shape, seed):
    import oracle_stoi as ost
    x, y = ost.gen_pair(3 + seed, shape[0])
    return dict(Y=x, e=y)


def _stoi_run(inp, checked=True):
    import oracle_stoi as ost
    from pb_bss_amd.evaluation import stoi
    return dict(stoi=np.asarray(stoi(inp['Y'], inp['e'], ost.FS)))


def _stoi_oracle(inp, out):
    """tests/test_gpu_stoi.py::check: ATOL = 1e-9"""
    import oracle_stoi as ost
    assert abs(float(out['stoi']) - float(ost.stoi(inp['Y'], inp['e'], ost.FS))) <= 1e-9


def _srmr_make(shape, seed):
    import oracle_srmr as osr
    return dict(Y=osr.speechlike(3 + seed, shape[0]))


def _srmr_run(inp, checked=True):
    from pb_bss_amd.evaluation import srmr
    return dict(srmr=np.asarray(srmr(inp['Y'])))


def _srmr_oracle(inp, out):
    """tests/test_gpu_srmr.py::check_values: RTOL = 1e-9"""
    import oracle_srmr as osr
    want = float(osr.srmr(inp['Y']))
    assert abs(float(out['srmr']) - want) <= 1e-9 * abs(want)


def _mask_make(shape, seed):
    import oracle_masks as om
    images = om.gen(seed, shape)
    return dict(Y=np.abs(images.astype(np.complex128)), images=images)


def _mask_run(inp, checked=True):
    from pb_bss_amd.extraction import mask_module
    return dict(quantile=_host(mask_module.quantile_mask(inp['Y'], (0.25, -0.5), axis=-2)),
                lorenz=_host(mask_module.lorenz_mask(inp['images'])))


def _mask_oracle(inp, out):
    """tests/test_gpu_mask_module.py::equal_masks: every entry equal, under the oracle's own
    condition that the thresholds are well determined"""
    import oracle_masks as om
    d = {}
    ref = om.quantile_mask(inp['Y'], (0.25, -0.5), axis=-2, details=d)
    om.assert_quantile_determined(d)
    assert (out['quantile'] == ref).all()
    d = {}
    ref = om.lorenz_mask(inp['images'].astype(np.complex128), details=d)
    om.assert_lorenz_determined(d)
    assert (out['lorenz'] == ref.astype(out['lorenz'].dtype)).all()


def _seed_make(shape, seed):
    import oracle_initializer as oi
    F, T, D, K = shape
    return dict(Y=oi.synth_case(F, T, D, K, seed), K=K)


def _seed_run(inp, checked=True):
    from pb_bss_amd.initializer.deflation import deflationSeed
    return dict(posterior=_host(deflationSeed(inp['Y'], inp['K'], permutation_free=True)))


def _seed_oracle(inp, out):
    """tests/test_gpu_initializer.py::compare: TOL = 1e-10, on well-determined input"""
    import oracle_initializer as oi
    details = {}
    ref = oi.deflation_seed(inp['Y'], inp['K'], details=details, permutation_free=True)
    oi.assert_well_determined(details)
    assert np.abs(out['posterior'] - ref).max() <= 1e-10


def _ccsg_make(shape, seed):
    import oracle_ccsg as oc
    B, N, D, K = shape
    return dict(Y=oc.frames(5 + seed, (B, N, D)), saliency=oc.saliency(5 + seed, (B, K, N)))


def _ccsg_run(inp, checked=True):
    from pb_bss_amd import engine
    return dict(covariance=_host(engine.ccsg_fit(_dev(inp['Y']), _dev(inp['saliency']))))


def _ccsg_oracle(inp, out):
    """tests/test_gpu_ccsg.py::check_covariance: (N + 4) eps of the largest diagonal entry,
    against the longdouble restatement"""
    import oracle_ccsg as oc
    want = oc.oracle_fit(inp['Y'], inp['saliency'], oc.fit_ext)
    N = inp['Y'].shape[-2]
    diag = np.einsum('...dd->...d', want).real.max(axis=-1).astype(np.float64)
    tol = (N + 4) * 2.0 ** -52 * diag[..., None, None]
    assert (np.abs(out['covariance'] - want).astype(np.float64) <= tol).all()


def _poison(key, index):
    return lambda inp: _nan_at(inp, key, index)


ROWS = {
    'em_plain': Row(
        ['pbbss_cacgmm_fit'], 'engine.em_fit',
        dict(small=(3, 130, 4, 3), big=(5, 200, 6, 4)), _make_stft,
        _em_fit(6, return_q=True), _em_oracle(6), _poison_frames, seeds=(63, 163)),
    'em_split': Row(
        ['pbbss_cacgmm_fit'], 'engine.em_fit, remainder bin as member workgroups',
        dict(small=_split_shape, big=_split_big), _make_stft,
        _em_fit(6, return_q=True), _em_oracle(6, tight_bins=_last_bins, tight_tol=1e-9),
        _poison_frames, seeds=(208, 308), xbuf='f64_split', timeout=_split_timeout),
    'em_split_f32': Row(
        ['pbbss_cacgmm_fit'], "engine.em_fit(precision='f32'), remainder bin",
        dict(small=_split_shape, big=_split_big), _make_stft,
        _em_fit(3, return_q=False, precision='f32'),
        _em_oracle(3, mask_tol=5e-4, weight_tol=None), _poison_frames,
        seeds=(208, 308), xbuf='f32_split'),
    'em_hbm': Row(
        ['pbbss_cacgmm_fit'], 'engine.em_fit, frames in the scratch slab',
        dict(small=(3, 1665, 8, 3), big=(4, 1800, 8, 4)), _make_stft,   # (D = 8 is the maximum)
        _em_fit(5, return_q=True), _em_oracle(5), _poison_frames, seeds=(70, 170)),
    'em_shared': Row(
        ['pbbss_cacgmm_fit_shared'], 'engine.em_fit_shared',
        dict(small=(3, 130, 4, 2), big=(5, 200, 6, 3)), _make_stft,
        _shared_run, _shared_oracle, _poison_frames, seeds=(62, 162), xbuf='cooperative',
        timeout=_shared_timeout),
    'em_generic': Row(
        ['pbbss_cacgmm_fit'], 'engine.em_fit, generic-size path',
        dict(small=(5, 70, 9, 2), big=(7, 100, 10, 3)), _make_stft,
        _em_fit(6, return_q=True), _em_oracle(6), _poison_frames, seeds=(11, 111)),
    'em_generic_parts': Row(
        ['pbbss_cacg_m_step', 'pbbss_cacgmm_predict'], 'engine.cacg_m_step, engine.em_predict',
        dict(small=(5, 70, 9, 2), big=(7, 100, 10, 3)), _generic_parts_make,
        _generic_parts_run, _generic_parts_oracle, _poison_frames, seeds=(11, 111)),
    'psd_hbm': Row(
        ['pbbss_psd'], 'engine.psd, frames in the scratch slab',
        dict(small=(3, 1665, 8, 3), big=(4, 1800, 8, 4)), _psd_make,
        _psd_run, _psd_oracle, _poison('X', (0, 0, 5)), seeds=(70, 170)),
    'cwmm_plain': Row(
        ['pbbss_cwmm_fit'], 'CWMMTrainer.fit_predict',
        dict(small=(3, 70, 4, 2), big=(5, 130, 5, 3)), _make_stft,
        _trainer_masks(_cwmm, 6), _cwmm_oracle, _poison_frames, seeds=(4, 104)),
    'cwmm_split': Row(
        ['pbbss_cwmm_fit'], 'CWMMTrainer.fit_predict, remainder bin',
        dict(small=lambda: (_cu_count() + 1, 128, 4, 2), big=lambda: (_cu_count() + 2, 200, 5, 3)),
        _make_stft, _trainer_masks(_cwmm, 6), _cwmm_oracle, _poison_frames,
        seeds=(32, 132), xbuf='watson_split', timeout=_cwmm_timeout),
    'cbmm': Row(
        ['pbbss_cbmm_fit'], 'CBMMTrainer.fit, .predict',
        dict(small=(4, 150, 3, 3), big=(5, 200, 4, 4)), _cbmm_make,
        _cbmm_run, _cbmm_oracle, _poison_frames, seeds=(24, 124)),
    'joint_gaussian': Row(
        ['pbbss_joint_fit'], 'GCACGMMTrainer.fit_predict (rotated loop, in-launch finalize)',
        dict(small=(3, 70, 4, 2, 12), big=(5, 130, 5, 3, 16)), _joint_make,
        _trainer_masks(_joint_trainer('gaussian'), 4), _joint_oracle('gaussian'), _poison_frames,
        seeds=(4, 104), xbuf='joint_finalize'),
    'joint_vmf': Row(
        ['pbbss_joint_fit'], 'VMFCACGMMTrainer.fit_predict (rotated loop, in-launch finalize)',
        dict(small=(3, 70, 4, 2, 12), big=(5, 130, 5, 3, 16)), _joint_make,
        _trainer_masks(_joint_trainer('vmf'), 4, max_concentration=80.),
        _joint_oracle('vmf', max_concentration=80.), _poison_frames, seeds=(4, 104),
        xbuf='joint_finalize'),
    'joint_inline_aligner': Row(
        ['pbbss_joint_fit'], 'GCACGMMTrainer.fit_predict(inline_permutation_alignment=True)',
        dict(small=(3, 70, 4, 2, 12), big=(5, 130, 5, 3, 16)), _joint_make,
        _trainer_masks(_joint_trainer('gaussian'), 4, weight_constant_axis=(-3,),
                       inline_permutation_alignment=True),
        _joint_oracle('gaussian', weight_constant_axis=(-3,), inline_permutation_alignment=True),
        _poison_frames, seeds=(4, 104)),
    'vmfmm': Row(
        ['pbbss_vmfmm_fit'], 'VMFMMTrainer.fit, .predict',
        dict(small=(1000, 2, 2), big=(1500, 5, 4)), _mixture_make(1.0, 0.7),
        _vmfmm_run, _vmfmm_oracle, _poison('Y', (7, 0)), seeds=(1002, 2002)),
    'vmfmm_wide': Row(
        ['pbbss_vmfmm_fit'], 'VMFMMTrainer.fit, .predict, K > 8 (class tiles of embed_wide)',
        dict(small=(4099, 3, 10), big=(4500, 5, 12)), _mixture_make(1.0, 0.7),
        _vmfmm_run, _vmfmm_oracle, _poison('Y', (7, 0)), seeds=(4112, 5112)),
    'gmm': Row(
        ['pbbss_gmm_fit'], "GMMTrainer.fit(covariance_type='spherical'), .predict",
        dict(small=(333, 5, 2), big=(500, 7, 4)), _mixture_make(2.0, 0.5),
        _gmm_run, _gmm_oracle, _poison('Y', (7, 0)), seeds=(335, 1335)),
    'gmm_wide': Row(
        ['pbbss_gmm_fit'], "GMMTrainer.fit(covariance_type='spherical'), K > 8",
        dict(small=(4099, 3, 10), big=(4500, 5, 12)), _mixture_make(2.0, 0.5),
        _gmm_run, _gmm_oracle, _poison('Y', (7, 0)), seeds=(4109, 5109)),
    'gmm_full': Row(
        ['pbbss_gmm_full_fit'], 'GMMTrainer.fit (full covariances), .predict',
        dict(small=(1000, 5, 3), big=(1500, 7, 4)), _mixture_make(1.5, 1.0),
        _gmm_full_run, _gmm_full_oracle, _poison('Y', (7, 0)), seeds=(8, 108)),
    'gmm_full_wide': Row(
        ['pbbss_gmm_full_fit'], 'GMMTrainer.fit (full covariances), K > 8',
        dict(small=(4099, 3, 10), big=(4500, 5, 12)), _mixture_make(1.5, 1.0),
        _gmm_full_run, _gmm_full_oracle, _poison('Y', (7, 0)), seeds=(9, 109)),
    'gaussian_spherical': Row(
        ['pbbss_embed_fit', 'pbbss_embed_log_pdf'],
        "GaussianTrainer.fit(covariance_type='spherical'), Gaussian.log_pdf",
        dict(small=(333, 5, 2), big=(500, 7, 4)), _single_make,
        _single_run('spherical'), _single_oracle('spherical'), _poison('Y', (7, 0)),
        seeds=(338, 1338)),
    'gaussian_full': Row(
        ['pbbss_gauss_full_fit', 'pbbss_gauss_full_log_pdf'],
        "GaussianTrainer.fit(covariance_type='full'), Gaussian.log_pdf",
        dict(small=(333, 5, 2), big=(500, 7, 4)), _single_make,
        _single_run('full'), _single_oracle('full'), _poison('Y', (7, 0)), seeds=(338, 1338)),
    'mixture_weight': Row(
        ['pbbss_estimate_mixture_weight'], 'engine.estimate_mixture_weight, summed over frames',
        dict(small=(3, 7, 4, 50), big=(4, 9, 5, 80)), _mixw_make,
        _mixw_run, _mixw_oracle, _poison('Y', (1, 2, 0, 3)), seeds=(1, 101)),
    'kmeans': Row(
        ['pbbss_kmeans_fit', 'pbbss_kmeans_predict', 'pbbss_kmeans_plusplus'],
        'KMeans.fit, BinaryGMM.predict, kmeans._call_plusplus (the seeding export)',
        dict(small=(63, 7, 2), big=(257, 40, 3)), _kmeans_make,
        _kmeans_run, _kmeans_oracle, _poison('Y', (7, 0)), seeds=(1, 2)),
    'dhtv_team_1': Row(
        ['pbbss_dhtv_calculate_mapping'], 'engine.dhtv_calculate_mapping, set_dhtv_team(1)',
        dict(small=(3, 33, 65), big=(4, 65, 130)), _dhtv_make,
        _dhtv_run(1), _dhtv_oracle, _poison('Y', (1, 0, 0, 3))),
    'dhtv_team_2': Row(
        ['pbbss_dhtv_calculate_mapping'], 'engine.dhtv_calculate_mapping, set_dhtv_team(2)',
        dict(small=(3, 33, 65), big=(4, 65, 130)), _dhtv_make,
        _dhtv_run(2), _dhtv_oracle, _poison('Y', (1, 0, 0, 3)), xbuf='dhtv_team',
        timeout=_dhtv_timeout(2)),
    'dhtv_team_-2': Row(
        ['pbbss_dhtv_calculate_mapping'], 'engine.dhtv_calculate_mapping, set_dhtv_team(-2)',
        dict(small=(3, 33, 65), big=(4, 65, 130)), _dhtv_make,
        _dhtv_run(-2), _dhtv_oracle, _poison('Y', (1, 0, 0, 3)), xbuf='dhtv_team_chunks',
        timeout=_dhtv_timeout(-2)),
    'inline_aligner': Row(
        ['pbbss_dhtv_calculate_mapping', 'pbbss_cacgmm_fit_shared'],
        'CACGMMTrainer.fit(inline_permutation_aligner=DHTVPermutationAlignment)',
        dict(small=(65, 150, 4, 2), big=(129, 200, 5, 3)), _make_stft,
        _aligner_run, _aligner_oracle, _poison_frames, seeds=(12, 112)),
    'wpe': Row(
        ['pbbss_wpe'], 'transform.wpe',
        dict(small=(2, 3, 1, 64), big=(3, 4, 2, 130)), _wpe_make,
        _wpe_run, _wpe_oracle, _poison('Y', (0, 0, 5))),
    'wpe_parts': Row(
        ['pbbss_wpe_power_inverse', 'pbbss_wpe_correlations'],
        'transform.get_power_inverse, transform.get_correlations',
        dict(small=(2, 3, 1, 64), big=(3, 4, 2, 130)), _wpe_make,
        _wpe_parts_run, _wpe_parts_oracle, _poison('Y', (0, 0, 5))),
    'istft': Row(
        ['pbbss_istft'], 'transform.istft',
        dict(small=(2, 37, 256, 64), big=(3, 50, 512, 128)), _istft_make,
        _istft_run, _istft_oracle, _poison('Y', (0, 3, 5))),
    'griffin_lim': Row(
        ['pbbss_griffin_lim'], 'transform.MISI(...).step(iterations=5)',
        dict(small=(3, 20, 64, 16), big=(4, 30, 128, 32)), _griffin_make,
        _griffin_run, _griffin_oracle, _poison('Y', (0, 3, 5)), seeds=GRIFFIN_SEEDS),
    'si_sdr': Row(
        ['pbbss_si_sdr', 'pbbss_signal_power'],
        'evaluation.si_sdr, sxr_module.get_variance_for_zero_mean_signal',
        dict(small=(3, 257), big=(5, 1000)), _si_sdr_make,
        _si_sdr_run, _si_sdr_oracle, _poison('e', (1, 7))),
    'sxr': Row(
        ['pbbss_input_sxr', 'pbbss_output_sxr'], 'sxr_module.input_sxr, sxr_module.output_sxr',
        dict(small=(3, 3, 4, 1000), big=(4, 4, 5, 1500)), _sxr_make,
        _sxr_run, _sxr_oracle, _poison('Y', (1, 0, 0, 7))),
    'bss_eval': Row(
        ['pbbss_bss_eval'], 'evaluation.mir_eval_sources',
        dict(small=(2, 2, 1000, 8), big=(3, 3, 1500, 24)), _bss_make,
        _bss_run, _bss_oracle(1e-9), _poison('e', (1, 7))),
    'bss_eval_host_solve': Row(
        ['pbbss_bss_eval', 'pbbss_bss_eval_system', 'pbbss_bss_eval_filters'],
        'evaluation.mir_eval_sources, singular Gram matrix: the host solves',
        dict(small=(3, 3, 1500, 24), big=(4, 4, 2500, 32)), _bss_dependent_make,
        _bss_run, _bss_oracle(1e-6), _poison('e', (1, 7))),
    'stoi': Row(
        ['pbbss_stoi'], 'evaluation.stoi',
        dict(small=(6000,), big=(9000,)), _stoi_make,
        _stoi_run, _stoi_oracle, _poison('e', (700,))),
    'srmr': Row(
        ['pbbss_srmr_vad', 'pbbss_srmr_energies'], 'evaluation.srmr (both work-slab sites)',
        dict(small=(4097,), big=(9001,)), _srmr_make,
        _srmr_run, _srmr_oracle, _poison('Y', (700,))),
    'threshold_masks': Row(
        ['pbbss_mask_quantile', 'pbbss_mask_lorenz'],
        'mask_module.quantile_mask, mask_module.lorenz_mask',
        dict(small=(3, 33, 150), big=(4, 65, 200)), _mask_make,
        _mask_run, _mask_oracle, _poison('Y', (1, 5, 7))),
    'deflation_seed': Row(
        ['pbbss_deflation_seed'], 'initializer.deflation.deflationSeed',
        dict(small=(257, 64, 4, 3), big=(513, 96, 6, 4)), _seed_make,
        _seed_run, _seed_oracle, _poison('Y', (5, 7, 0)), seeds=(0, 1)),
    'ccsg_fit': Row(
        ['pbbss_ccsg_fit'], 'engine.ccsg_fit',
        dict(small=(2, 300, 4, 2), big=(3, 600, 6, 3)), _ccsg_make,
        _ccsg_run, _ccsg_oracle, _poison('Y', (0, 5, 0))),
}

# export name -> the rows whose Python call reaches it
FAMILIES = {}
for _name, _row in ROWS.items():
    for _export in _row.exports:
        FAMILIES.setdefault(_export, []).append(_name)

# exports that take no memory from the handle's slabs, control buffers or team buffer, by group
NO_HANDLE_MEMORY = {
    'host functions without a handle, and the handle itself': {
        'pbbss_version', 'pbbss_error_string', 'pbbss_create', 'pbbss_destroy',
        'pbbss_shard_bounds', 'pbbss_stft_num_frames', 'pbbss_bss_eval_workspace',
        'pbbss_comm_unique_id'},
    'settings and read-outs of the handle (pbbss_split_error / _reset read and zero the flag '
    'words of xbuf; they carve nothing and are part of every sequence here)': {
        'pbbss_set_timing', 'pbbss_last_kernel_ms', 'pbbss_kernel_ms_lagged',
        'pbbss_set_phase_profile', 'pbbss_set_split_tail', 'pbbss_split_error',
        'pbbss_split_reset', 'pbbss_set_spin_limit', 'pbbss_set_dhtv_team', 'pbbss_set_dhtv_probe',
        'pbbss_bss_eval_phase_ms'},
    'the communicator: its pack buffers are its own, grown by the gather and released by '
    'pbbss_comm_destroy (tests/test_gpu_comm.py); more than one GPU is another test': {
        'pbbss_comm_create', 'pbbss_comm_destroy', 'pbbss_comm_info', 'pbbss_allgather_masks',
        'pbbss_allgather_unpack'},
    'one launch (or a fixed chain) from the caller\'s inputs to the caller\'s outputs, working '
    'storage in LDS / registers or handed in by the caller': {
        'pbbss_normalize_observation', 'pbbss_heev_batched', 'pbbss_gev', 'pbbss_gev_general',
        'pbbss_solve', 'pbbss_mvdr_souden', 'pbbss_mvdr', 'pbbss_ban',
        'pbbss_apply_beamforming_vector', 'pbbss_apply_beamforming_vector_shared',
        'pbbss_select_reference_channel', 'pbbss_wmwf', 'pbbss_lcmv', 'pbbss_phase_correction',
        'pbbss_snr_postfilter', 'pbbss_reference_channel_terms', 'pbbss_rank_one_approximation',
        'pbbss_matvec', 'pbbss_distortionless_normalization', 'pbbss_zero_degree_normalization',
        'pbbss_condition_covariance', 'pbbss_apply_online_beamforming_vector',
        'pbbss_apply_mapping', 'pbbss_pa_pairwise_mapping', 'pbbss_pa_compose_mapping',
        'pbbss_pa_mapping_from_scores', 'pbbss_cbingham_find_eigenvalues',
        'pbbss_log_pdf_to_affiliation', 'pbbss_log_pdf_to_affiliation_inline_pa', 'pbbss_stft',
        'pbbss_mask_pointwise', 'pbbss_gammatone', 'pbbss_srmr_score', 'pbbss_resample_poly',
        'pbbss_ccsg_log_pdf', 'pbbss_wpe_filter_matrix', 'pbbss_wpe_apply_filter'},
    'frame-recursive kernels: their state lives in tensors of the caller': {
        'pbbss_wpe_online', 'pbbss_online_mvdr', 'pbbss_online_cacgmm'},
}

# row -> the call-to-call difference measured where two calls on one input on one handle are NOT
# bit-identical (such a row is compared with its oracle after every sequence instead of with R0)
NOT_REPRODUCIBLE = {}

# The rows whose workgroups keep control words in memory of the handle that outlives the launch:
# the conventions of the first 256 bytes of xbuf, and the two DHTV team kernels (frame slices and
# bin chunks; their barriers' words are in team_buf).  'dhtv_team_1' is the one-workgroup kernel:
# no barrier, no control word, nothing shared -- it is an ordinary row of P1 .. P5.
XBUF_ROWS = [name for name, row in ROWS.items() if row.xbuf]
TIMEOUT_ROWS = [name for name, row in ROWS.items() if row.timeout]


# ---- the comparisons ---------------------------------------------------------------------------
_R0 = {}


def r0(name):
    """The result of the row as the first call of a fresh handle, and the result of the same call
    repeated on that handle; computed once, shared, read-only."""
    if name not in _R0:
        row = ROWS[name]
        with fresh_handle():
            first = row.run(row.inputs())
            again = row.run(row.inputs())
            _assert_no_split_error(name)
        _frozen(*first.values())
        _frozen(*again.values())
        _R0[name] = (first, again)
    return _R0[name]


def _assert_no_split_error(what):
    from pb_bss_amd import engine
    assert engine.split_error() == 0, what


def _assert_equals_r0(name, got, state):
    row = ROWS[name]
    if name in NOT_REPRODUCIBLE:
        row.oracle(row.inputs(), got)
        return
    worst = _largest_difference(got, r0(name)[0])
    print(f'{name} after {state}: largest difference against R0 '
          f'{max((w[0] for w in worst.values()), default=0.0):.3e}')
    assert not worst, (name, state, worst)


def _unchecked(row, inp):
    """Run the row without acting on its status words.  Where the call has no such switch the
    Python layer raises AFTER every kernel of the call has been enqueued and its status read back:
    what the handle's memory holds then is what an unchecked call leaves."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with np.errstate(all='ignore'):
            try:
                row.run(inp, False)
            except _status_errors():
                pass


def _refused_calls():
    """tests/test_gpu_capi_errors.py::test_invalid_arguments_return_codes_not_crashes: a shape
    beyond the kernels (UNSUPPORTED), bad options and a missing pointer (INVALID_ARG), an
    embedding wider than 256 (UNSUPPORTED).  They are refused by the argument checks of
    pbbss_cacgmm_fit and pbbss_embed_log_pdf, in front of any carving: what P5 pins is that a
    refusal leaves the handle as it was, for whichever row follows; it does not reach the row's own
    export.  No argument set there (or anywhere in the suite) ends in PBBSS_ERR_LDS_CAPACITY on
    this device: an utterance too long for LDS is served by the kernel variants that keep the
    frames in the scratch slab, so that code has no sequence here."""
    import torch
    from pb_bss_amd import _lib
    device = torch.cuda.current_device()          # the device fresh_handle() keys on
    lib, h, stream = _lib.load(), _lib.handle(device), _lib.stream_ptr(device)
    B, T, D, K = 3, 40, 4, 2
    y = torch.zeros((B, T, D), dtype=torch.complex64, device='cuda')
    g = torch.full((B, K, T), 0.5, dtype=torch.float64, device='cuda')
    vec = torch.zeros((B, K, D, D), dtype=torch.complex128, device='cuda')
    val = torch.zeros((B, K, D), dtype=torch.float64, device='cuda')
    w = torch.zeros((B, K), dtype=torch.float64, device='cuda')
    st = torch.zeros((B, K), dtype=torch.int32, device='cuda')
    opts = _lib.EmOpts(iterations=2, covariance_norm=1, weight_mode=0, layout=0,
                       affiliation_eps=1e-10, eigenvalue_floor=1e-10)

    def fit(gg=g, KK=K, DD=D, o=opts):
        return lib.pbbss_cacgmm_fit(h, _lib.ptr(y), B, T, DD, KK, _lib.ptr(gg), None, None, None,
                                    None, None, ctypes.byref(o), _lib.ptr(vec), _lib.ptr(val),
                                    _lib.ptr(w), _lib.ptr(st), None, None, stream)
    assert fit(DD=35) == _lib.ERR_UNSUPPORTED
    assert fit(KK=20) == _lib.ERR_UNSUPPORTED
    assert fit(gg=None) == _lib.ERR_INVALID_ARG
    assert fit(o=_lib.EmOpts(iterations=0, covariance_norm=1)) == _lib.ERR_INVALID_ARG
    assert fit(o=_lib.EmOpts(iterations=1, covariance_norm=7)) == _lib.ERR_INVALID_ARG
    e = torch.zeros((1, 10, 300), dtype=torch.float32, device='cuda')
    m = torch.zeros((1, 2, 300), dtype=torch.float64, device='cuda')
    s = torch.ones((1, 2), dtype=torch.float64, device='cuda')
    o = torch.zeros((1, 2, 10), dtype=torch.float64, device='cuda')
    assert lib.pbbss_embed_log_pdf(h, _lib.ptr(e), 0, 1, 10, 300, 2, 0, _lib.ptr(m), _lib.ptr(s),
                                   _lib.ptr(o), stream) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()


@pytest.mark.parametrize('name', list(ROWS))
def test_first_call_of_a_fresh_handle_matches_the_oracle_and_repeats(name):
    """R0 against the float64 oracle at the tolerance of the family's own test (cited in the
    docstring of the row's oracle function), so that "equally wrong every time" does not pass;
    and the precondition of everything below: a second call on the same input is bit-identical."""
    row = ROWS[name]
    first, again = r0(name)
    row.oracle(row.inputs(), first)
    worst = _largest_difference(again, first)
    print(f'{name}: two calls on one input differ by {worst or 0}')
    if name in NOT_REPRODUCIBLE:
        row.oracle(row.inputs(), again)
    else:
        assert not worst, (name, worst)


@pytest.mark.parametrize('name', list(ROWS))
def test_after_the_same_call_on_other_data_and_at_a_larger_shape(name):
    """P1 and P2, one after the other on one fresh handle (P2 regrows the slabs that P1 filled)"""
    row = ROWS[name]
    want_first = r0(name)
    assert want_first is not None
    with fresh_handle():
        row.run(row.inputs('small', 1))
        _assert_equals_r0(name, row.run(row.inputs()), 'P1 other data')
        row.run(row.inputs('big', 1))
        _assert_equals_r0(name, row.run(row.inputs()), 'P2 larger shape')
        _assert_no_split_error(name)


@pytest.mark.parametrize('name', list(ROWS))
def test_after_one_call_of_every_other_family(name):
    """P3: every other row of the table once (every other user of the work and scratch slabs, of
    xbuf and of the team buffer), then this one"""
    row = ROWS[name]
    r0(name)
    with fresh_handle():
        for other, other_row in ROWS.items():
            if other != name:
                other_row.run(other_row.inputs())
        _assert_equals_r0(name, row.run(row.inputs()), 'P3 every other family')
        _assert_no_split_error(name)


@pytest.mark.parametrize('first,second', [
    (a, b) for a in XBUF_ROWS for b in XBUF_ROWS if ROWS[a].xbuf != ROWS[b].xbuf])
def test_ordered_pairs_of_the_xbuf_families(first, second):
    """P3 for the conventions that share the first 256 bytes of xbuf: arrival counters that the
    last member puts back to zero (float64, packed-FP32 and Watson split groups), the value 1
    behind a 64-byte memset at +128 (cooperative launches), the free word at +224 (in-launch
    joint finalize), and the DHTV team kernel's control words beside them.  (A family behind
    itself is P1.)"""
    r0(second)
    with fresh_handle():
        ROWS[first].run(ROWS[first].inputs())
        _assert_equals_r0(second, ROWS[second].run(ROWS[second].inputs()), f'P3 {first}')
        _assert_no_split_error((first, second))


@pytest.mark.parametrize('name', list(ROWS))
def test_after_a_non_finite_input_and_after_refused_calls(name):
    """P4: the same call on an input with one NaN, its status bits set and not acted on; then the
    clean input.  P5: calls the library refuses, then the clean input."""
    row = ROWS[name]
    r0(name)
    with fresh_handle():
        _unchecked(row, row.poison(row.inputs()))
        _assert_equals_r0(name, row.run(row.inputs()), 'P4 non-finite input')
        _refused_calls()
        _assert_equals_r0(name, row.run(row.inputs()), 'P5 refused calls')
        _assert_no_split_error(name)


@pytest.fixture
def one_poll():
    """tests/test_gpu_timeouts.py::one_poll, on the handle current when the test body runs"""
    from pb_bss_amd import engine
    yield engine
    engine.set_spin_limit(0)
    engine.split_reset()
    engine.set_split_tail(True)


@pytest.mark.parametrize('name', TIMEOUT_ROWS)
def test_after_a_time_out_that_the_engine_consumed(name, one_poll):
    """P6: with one poll allowed per bounded wait the family of the row runs through its checked
    entry point at the shape at which tests/test_gpu_timeouts.py makes the same wait give up.  The
    time-out is ASSERTED: the entry point reports it with the family's RuntimeWarning, consumes it
    (pbbss_split_error back at 0) and repeats the work on the path without inter-workgroup waits.
    With the limit back at 0, every OTHER family of XBUF_ROWS equals its R0, and so does the row
    itself, at its small shape.

    'em_split_f32' has no P6 of its own: the launcher of the packed-FP32 kernel
    (csrc/em32_inst.hip) does not hand the handle's spin limit to the kernel, so its split groups
    always wait with the default of about two seconds and cannot be made to give up with the knob;
    only starving the device would do it.  The row is compared behind every other family's
    time-out."""
    engine = one_poll
    row = ROWS[name]
    others = [other for other in XBUF_ROWS if ROWS[other].xbuf != row.xbuf]
    for other in others + [name]:
        r0(other)
    with fresh_handle():
        engine.split_reset()
        engine.set_spin_limit(1)
        with pytest.warns(RuntimeWarning, match=row.timeout.match):
            row.timeout()
        assert engine.split_error() == 0          # consumed
        engine.set_spin_limit(0)
        for other in others + [name]:
            _assert_equals_r0(other, ROWS[other].run(ROWS[other].inputs()), f'P6 {name}')
        _assert_no_split_error(name)


# ---- stream order on one handle --------------------------------------------------------------------
def _generic_100(inp):
    """(upload, call): 100 iterations of the generic-size loop, three kernels each"""
    from pb_bss_amd import engine
    K = inp['init'].shape[-2]
    y, g = _dev(inp['Y']), _dev(inp['init'])
    return lambda: engine.em_fit(y, K, gamma0=g, iterations=100, final_predict=True,
                                 check_status=False)


def _wpe_device(inp):
    """40 iterations, four kernels each: long enough to be running when the next call arrives"""
    from pb_bss_amd import engine
    y = _dev(inp['Y'])
    return lambda: engine.wpe(y, inp['taps'], inp['delay'], 40)


def _joint_device(inp):
    from pb_bss_amd import _lib, engine
    K = inp['init'].shape[-2]
    y, e, g = _dev(inp['Y']), _dev(inp['e']), _dev(inp['init'])
    return lambda: engine.joint_fit(y, e, K, _lib.EMBED_GAUSS_SPHERICAL, gamma0=g, iterations=40,
                                    final_predict=True, check_status=False)


def _kmeans_device(inp):
    from pb_bss_amd.distribution import kmeans
    xd, centers = _dev(inp['Y'][None]), _dev(inp['init'][None])
    return lambda: kmeans._call_fit(xd, inp['init'].shape[0], None, centers, 300, 1e-4,
                                    kmeans.DEFAULT_BLOCK)


def _flat(result):
    values = result.values() if isinstance(result, dict) else result
    return [_host(v) for v in values if v is not None]


@pytest.mark.parametrize('first,second', [('em_generic', 'wpe'), ('wpe', 'em_generic'),
                                          ('joint_gaussian', 'kmeans')])
def test_two_streams_on_one_handle(first, second):
    """One thread, two torch streams, one handle: a long call on the first stream (100 iterations
    of the generic-size EM loop are 300 kernels on the work slab) and AT ONCE a call on the second
    stream that carves the head of the same slab.  `_lib.launch` makes the second stream wait for
    the first, so each result equals, bit for bit, the result of that call made alone.

    A regression test: with the ordering in place it passes deterministically; were the ordering
    removed, the two calls would overlap on the device and corrupt each other's workspace with
    high probability, not with certainty (measured once, with an ordering that never started
    because torch.Stream answers False to `!= None`: five of six such pairs left a whole bin of the
    EM result wrong, masks off by up to 1.0, status FLOORED)."""
    import torch
    calls = {'em_generic': _generic_100, 'wpe': _wpe_device, 'joint_gaussian': _joint_device,
             'kmeans': _kmeans_device}
    with fresh_handle():
        # the inputs are on the device before anything is timed against anything: between the two
        # stream blocks the host only allocates the outputs of the second call and enqueues it
        call_a, call_b = calls[first](ROWS[first].inputs()), calls[second](ROWS[second].inputs())
        torch.cuda.synchronize()
        alone_a = _flat(call_a())
        torch.cuda.synchronize()
        alone_b = _flat(call_b())
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            got_a = call_a()
        with torch.cuda.stream(s2):
            got_b = call_b()
        s1.synchronize()
        s2.synchronize()
        torch.cuda.synchronize()
        got_a, got_b = _flat(got_a), _flat(got_b)
        _assert_no_split_error((first, second))
    for got, alone, what in ((got_a, alone_a, first), (got_b, alone_b, second)):
        assert len(got) == len(alone)
        for g, w in zip(got, alone):
            assert _bits(g) == _bits(w), what
