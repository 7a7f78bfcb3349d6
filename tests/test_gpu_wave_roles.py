"""GPU: who does what inside an EM workgroup, iteration by iteration.

The persistent EM loops hand their per-iteration roles (which 64-frame chunks of the E phase,
which share of the Hermitian entries in the M phase, which classes to factor) to the four waves
of a workgroup through a role index; in the full workgroups of the float64 and the packed-FP32
kernel it moves on by one wave per iteration (em_role, csrc/pbbss_dev.hpp), in the member
workgroups of a remainder bin and in the shared-weight kernel it is the wave index.  A wrong role
map shows as a chunk of frames that nobody updates, a slot of the cross-wave sums that nobody
writes, or a class that is factored twice or never -- all of which move the masks by far more
than rounding.  The shapes below are the smallest at which each of these can happen: iteration
counts on both sides of a full turn of the four roles, frame counts that leave one, two or three
roles without an E chunk, every number of classes per role, the kernel variant with the frames in
HBM, the member workgroups of a remainder bin, the shared-weight kernel and the packed-FP32
kernel.

Reference: the float64 oracle (oracle/cacgmm.py) on the complex128 upcast of the same values, at
the tolerances tests/test_gpu_em.py uses for the same quantity and iteration count (one step:
mask 1e-9, weight 1e-14; trajectories of 2 .. 20 iterations: mask 1e-7, weight 1e-8; split groups
against plain launches: 1e-10 relative; packed FP32: those of tests/test_gpu_f32.py)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    from pb_bss_amd import _lib
    return _lib.to_device(x, dtype)


def _host(x):
    from pb_bss_amd import _lib
    return _lib.to_host(x)


@functools.lru_cache(maxsize=None)
def _problem(F, T, D, K, seed):
    from pb_bss_amd.testing import synth
    Y, init = synth.make_stft(F, T, D, K, seed=seed)
    Y.setflags(write=False)
    init.setflags(write=False)
    return Y, init


@functools.lru_cache(maxsize=None)
def _oracle(F, T, D, K, seed, iterations):
    """(model, masks) of the oracle; computed once per shape, shared and read-only"""
    from oracle import cacgmm as oc
    Y, init = _problem(F, T, D, K, seed)
    Y128 = Y.astype(np.complex128)
    m = oc.em_fit(Y128, init, iterations=iterations)
    mask = oc.em_predict(m, Y128)
    mask.setflags(write=False)
    return m, mask


def _fit(Y, init, iterations, return_q=True, **kw):
    from pb_bss_amd import engine
    return engine.em_fit(_dev(Y), init.shape[-2], gamma0=_dev(init), iterations=iterations,
                         final_predict=True, return_q=return_q, **kw)


def _check(r, m, mask, iterations):
    mask_tol, weight_tol = (1e-9, 1e-14) if iterations == 1 else (1e-7, 1e-8)
    assert (_host(r['status']) & 3 == 0).all(), _host(r['status'])  # no failure bit
    aff = _host(r['affiliation'])
    assert np.isfinite(aff).all()
    err = np.abs(aff - mask).max()
    werr = np.abs(_host(r['weight'])[..., None] - m['weight']).max()
    print(f'mask err {err:.3e} weight err {werr:.3e}')
    assert err < mask_tol, err
    assert werr < weight_tol, werr


@pytest.mark.parametrize('D', [8, 2])
@pytest.mark.parametrize('iterations', [1, 2, 4, 5, 9])
def test_iteration_counts_around_a_full_turn(iterations, D):
    """One turn, a full turn of the four roles, the wrap, two wraps plus one.  T = 300 is five
    chunks of 64 frames: one role owns two E chunks, the others one."""
    F, T, K, seed = 3, 300, 3, 40 + D
    Y, init = _problem(F, T, D, K, seed)
    m, mask = _oracle(F, T, D, K, seed, iterations)
    _check(_fit(Y, init, iterations), m, mask, iterations)


@pytest.mark.parametrize('T', [64, 65, 129, 257])
def test_roles_without_an_e_chunk(T):
    """1, 2, 3 and 5 chunks: roles that own no E chunk land on every wave in turn, and still have
    to write their slot of the cross-wave class sums."""
    F, D, K, seed, iterations = 3, 8, 3, 50 + T, 5
    Y, init = _problem(F, T, D, K, seed)
    m, mask = _oracle(F, T, D, K, seed, iterations)
    _check(_fit(Y, init, iterations), m, mask, iterations)


@pytest.mark.parametrize('K', [1, 2, 4, 5, 6])
def test_classes_per_role(K):
    """One role factors (K = 1, 2), all four do (K = 4), two classes on one role (K = 5, 6)."""
    F, T, D, seed, iterations = 3, 130, 4, 60 + K, 6
    Y, init = _problem(F, T, D, K, seed)
    m, mask = _oracle(F, T, D, K, seed, iterations)
    _check(_fit(Y, init, iterations), m, mask, iterations)


@pytest.mark.parametrize('K', [2, 4, 5])
def test_fit_from_a_model_runs_the_e_phase_in_iteration_zero(K):
    from oracle import cacgmm as oc
    from pb_bss_amd import engine
    F, T, D, seed, iterations = 3, 130, 4, 60 + K, 6
    Y, init = _problem(F, T, D, K, seed)
    Y128 = Y.astype(np.complex128)
    start = oc.em_fit(Y128, init, iterations=2)
    m = oc.em_fit(Y128, start, iterations=iterations)
    mask = oc.em_predict(m, Y128)
    model = (_dev(start['eigvec']), _dev(start['eigval']),
             _dev(np.ascontiguousarray(start['weight'][..., 0])))
    r = engine.em_fit(_dev(Y), K, model=model, iterations=iterations, final_predict=True)
    _check(r, m, mask, iterations)


@pytest.mark.parametrize('K', [2, 6])
def test_saliency(K):
    from oracle import cacgmm as oc
    F, T, D, seed, iterations = 3, 130, 4, 60 + K, 6
    Y, init = _problem(F, T, D, K, seed)
    sal = np.random.default_rng(K).uniform(0.0, 1.0, size=(F, T))
    sal[:, ::7] = 0.0
    Y128 = Y.astype(np.complex128)
    m = oc.em_fit(Y128, init, iterations=iterations, saliency=sal)
    mask = oc.em_predict(m, Y128)
    _check(_fit(Y, init, iterations, saliency=_dev(sal)), m, mask, iterations)


@pytest.mark.parametrize('K', [2, 4])
def test_shared_weight_kernel(K):
    """weight_constant_axis=(-3, -1): the cooperative kernel, all bins of the utterance resident"""
    from oracle import cacgmm as oc
    from pb_bss_amd import _lib, engine
    F, T, D, seed, iterations = 3, 130, 4, 60 + K, 6
    Y, init = _problem(F, T, D, K, seed)
    Y128 = Y.astype(np.complex128)
    m = oc.em_fit(Y128, init, iterations=iterations, weight_constant_axis=(-3, -1))
    mask = oc.em_predict(m, Y128)
    r = engine.em_fit_shared(_dev(Y), K, F, weight_mode=_lib.WEIGHT_SHARED_K, gamma0=_dev(init),
                             iterations=iterations, final_predict=True)
    assert r is not None, 'the cooperative kernel serves three small bins'
    assert (_host(r['status']) & 3 == 0).all()
    err = np.abs(_host(r['affiliation']) - mask).max()
    werr = np.abs(_host(r['weight']).reshape(K) - np.asarray(m['weight']).reshape(K)).max()
    print(f'mask err {err:.3e} weight err {werr:.3e}')
    assert err < 1e-7, err
    assert werr < 1e-8, werr


def test_frames_in_hbm_variant():
    """complex64, D = 8, K = 3: 96 bytes of LDS per frame and ~3.7 KB beside them -- 1664 frames
    (26 chunks) fit the 160 KB of a compute unit, 1665 (27 chunks) select the variant that keeps
    the frame arrays in an HBM / L2 slab."""
    F, T, D, K, seed, iterations = 3, 1665, 8, 3, 70, 5
    Y, init = _problem(F, T, D, K, seed)
    m, mask = _oracle(F, T, D, K, seed, iterations)
    _check(_fit(Y, init, iterations), m, mask, iterations)


def _cu_count():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@functools.lru_cache(maxsize=None)
def _split_problem(T):
    return _problem(_cu_count() + 1, T, 2, 3, 80 + T)


@pytest.mark.parametrize('T', [128, 200])
def test_member_workgroups_of_the_remainder_bin(T):
    """One bin more than compute units: the last bin runs as member workgroups with 64-frame
    windows (T = 128: two members, fewer than classes -- every member factors every class;
    T = 200: four members -- member k factors class k).  Against the same problems fitted in
    launches of at most one bin per compute unit."""
    from oracle import cacgmm as oc
    from pb_bss_amd import engine
    iterations = 6
    Y, init = _split_problem(T)
    cu = Y.shape[0] - 1
    split = _fit(Y, init, iterations)
    assert engine.split_error() == 0
    head = _fit(Y[:cu], init[:cu], iterations)
    tail = _fit(Y[cu:], init[cu:], iterations)
    assert engine.split_error() == 0
    assert (_host(split['status']) & 3 == 0).all()
    for key in ('affiliation', 'eigval', 'weight', 'quadratic_form'):
        ref = np.concatenate([_host(head[key]), _host(tail[key])])
        err = np.abs(_host(split[key]) - ref).max()
        print(f'{key}: split vs plain {err:.3e}')
        assert err < 1e-10 * max(1.0, np.abs(ref).max()), key
    Y128 = Y[-2:].astype(np.complex128)
    mask = oc.em_predict(oc.em_fit(Y128, init[-2:], iterations=iterations), Y128)
    assert np.abs(_host(split['affiliation'])[-2:] - mask).max() < 1e-9


def _fit32(Y, init, iterations):
    r = _fit(Y, init, iterations, return_q=False, precision='f32')  # (no quadratic form in f32)
    return {k: (None if v is None else _host(v)) for k, v in r.items()}


def test_packed_fp32_kernel_against_the_oracle():
    """tests/test_gpu_f32.py: two iterations against the float64 oracle, 2e-4"""
    F, T, D, K, seed, iterations = 3, 300, 8, 3, 48, 2
    Y, init = _problem(F, T, D, K, seed)
    m, mask = _oracle(F, T, D, K, seed, iterations)
    r = _fit32(Y, init, iterations)
    err = np.abs(r['affiliation'] - mask).max()
    print(f'mask err {err:.3e}')
    assert err < 2e-4, err
    assert int(r['status'].max()) & 3 == 0


def test_packed_fp32_members_of_the_remainder_bin():
    """tests/test_gpu_f32.py: three iterations; the bins in front of the remainder bin equal the
    plain launch bit for bit, the remainder bin to float32 rounding, the oracle at 5e-4"""
    from oracle import cacgmm as oc
    from pb_bss_amd import engine
    iterations = 3
    Y, init = _split_problem(128)
    cu = Y.shape[0] - 1
    split = _fit32(Y, init, iterations)
    assert engine.split_error() == 0
    head = _fit32(Y[:cu], init[:cu], iterations)
    tail = _fit32(Y[cu:], init[cu:], iterations)
    assert np.abs(split['affiliation'][:cu] - head['affiliation']).max() == 0.0
    err = np.abs(split['affiliation'][cu:] - tail['affiliation']).max()
    print(f'remainder bin, split vs plain {err:.3e}')
    assert err < 1e-4, err
    sel = [0, cu - 1, cu]
    Y128 = Y[sel].astype(np.complex128)
    ref = oc.em_predict(oc.em_fit(Y128, init[sel], iterations=iterations), Y128)
    assert np.abs(split['affiliation'][sel] - ref).max() < 5e-4
    assert int(split['status'].max()) & 3 == 0


def test_two_fits_of_one_input_are_bitwise_equal():
    F, T, D, K, seed, iterations = 3, 300, 8, 3, 48, 9
    Y, init = _problem(F, T, D, K, seed)
    a = _host(_fit(Y, init, iterations)['affiliation'])
    b = _host(_fit(Y, init, iterations)['affiliation'])
    assert np.array_equal(a, b)
