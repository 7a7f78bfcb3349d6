"""CPU: host-side logic of the drop-in layer that needs no GPU."""
import os

import numpy as np
import pytest

from oracle import cacgmm as oc


def test_host_mixture_weight_formula_and_no_cpu_fallback():
    """`_host_estimate_mixture_weight` is the formula for the axis sets the reduction kernel does
    not serve (a handful of axes, off the hot path): checked against the oracle.  The PUBLIC
    helpers are device steps since round 6 (tests/test_gpu_golden.py pins them to the reference's
    outputs) and must fail loudly on a box without a GPU instead of computing on the host."""
    import torch
    from pb_bss_amd.distribution.mixture_model_utils import (
        _host_estimate_mixture_weight, estimate_mixture_weight, log_pdf_to_affiliation)
    a = np.array([[0.4, 1, 0.4], [0.6, 0, 0.6]])
    assert np.allclose(_host_estimate_mixture_weight(a, None, -1), [[0.6], [0.4]])
    assert np.allclose(estimate_mixture_weight(a, weight_constant_axis=-2), [[0.5], [0.5]])
    rng = np.random.default_rng(0)
    aff = rng.uniform(size=(4, 3, 10))
    sal = rng.uniform(size=(4, 10))
    for ax in [-1, (-1,), (-3,), (-3, -1)]:
        assert np.allclose(_host_estimate_mixture_weight(aff, sal, ax),
                           oc.estimate_mixture_weight(aff, sal, ax))
        assert np.allclose(_host_estimate_mixture_weight(aff, None, ax),
                           oc.estimate_mixture_weight(aff, None, ax))
    if not torch.cuda.is_available():
        lp = rng.standard_normal((4, 3, 10)) * 50
        w = rng.uniform(size=(4, 3, 1))
        with pytest.raises(RuntimeError):
            log_pdf_to_affiliation(w, lp)
        with pytest.raises(RuntimeError):
            estimate_mixture_weight(aff, sal, -1)


def test_weight_mode_mapping():
    from pb_bss_amd import _lib
    from pb_bss_amd.distribution.cacgmm import CACGMMTrainer
    wm = CACGMMTrainer._weight_mode
    assert wm((-1,), 3) == _lib.WEIGHT_PER_CLASS_MEAN
    assert wm(-1, 3) == _lib.WEIGHT_PER_CLASS_MEAN
    assert wm(2, 3) == _lib.WEIGHT_PER_CLASS_MEAN
    assert wm(-2, 3) == _lib.WEIGHT_UNIFORM
    assert wm(1, 3) == _lib.WEIGHT_UNIFORM
    assert wm((-3,), 3) is None
    assert wm((-3, -1), 3) is None
    assert wm(-3, 3) is None


def test_shared_weight_mode_mapping():
    """weight_constant_axis sets that average the weights over the last independent axis (the
    frequency bins) go to the cooperative kernel (pbbss_cacgmm_fit_shared); everything else that
    couples bins stays with the step-wise loop."""
    from pb_bss_amd import _lib
    from pb_bss_amd.distribution.cacgmm import CACGMMTrainer
    sm = CACGMMTrainer._shared_mode
    assert sm((-3,), 3) == _lib.WEIGHT_SHARED_KT
    assert sm(-3, 3) == _lib.WEIGHT_SHARED_KT
    assert sm((0,), 3) == _lib.WEIGHT_SHARED_KT
    assert sm((-3, -1), 3) == _lib.WEIGHT_SHARED_K
    assert sm([-1, -3], 4) == _lib.WEIGHT_SHARED_K
    assert sm((1, 3), 4) == _lib.WEIGHT_SHARED_K            # positive axes of a (U, F, K, T) posterior
    assert sm((-1,), 3) is None and sm(-2, 3) is None        # per-bin modes: the fused kernel
    assert sm((-4,), 4) is None and sm((-4, -3), 4) is None  # over utterances: step-wise loop
    assert sm((-3,), 2) is None                              # no independent axis at all
    assert _lib.WEIGHT_SHARED_K == 2 and _lib.WEIGHT_SHARED_KT == 3  # include/pbbss.h
    header = open(__import__('os').path.join(
        __import__('os').path.dirname(__import__('os').path.dirname(__file__)), 'include', 'pbbss.h')).read()
    assert '#define PBBSS_WEIGHT_SHARED_K 2' in header and '#define PBBSS_WEIGHT_SHARED_KT 3' in header


def test_model_containers_roundtrip():
    from pb_bss_amd.distribution import CACGMM, ComplexAngularCentralGaussian
    m = CACGMM(weight=np.ones((2, 1)),
               cacg=ComplexAngularCentralGaussian(np.eye(2)[None].repeat(2, 0), np.ones((2, 2))))
    d = m.to_dict()
    assert set(d) == {'weight', 'cacg'} and set(d['cacg']) == {
        'covariance_eigenvectors', 'covariance_eigenvalues'}
    m2 = CACGMM.from_dict({'weight': d['weight'],
                           'cacg': ComplexAngularCentralGaussian.from_dict(d['cacg'])})
    assert np.allclose(m2.cacg.covariance, m.cacg.covariance)
    assert np.allclose(m.cacg.log_determinant, 0)
    try:
        m.cacg.covariances
    except AttributeError as e:
        assert 'Close matches' in str(e) and 'covariance_eigenvalues' in str(e)
    else:
        raise AssertionError('expected AttributeError')


def test_synth_is_deterministic():
    from oracle import synth
    a = synth.make_stft(3, 10, 4, 2, seed=1)
    b = synth.make_stft(3, 10, 4, 2, seed=1)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    assert a[0].dtype == np.complex64 and a[1].dtype == np.float64
    assert np.allclose(a[1].sum(axis=1), 1)


def test_beamformer_recipe_parser():
    """get_bf_vector's recipe grammar (reference dispatch: beamformer_wrapper.py:160-226)."""
    from pb_bss_amd.extraction.beamformer_wrapper import _parse
    assert _parse('pca') == ('pca', None, None)
    assert _parse('ch3') == ('channel', 3, None)
    assert _parse('pca+mvdr') == ('atf_mvdr', 'pca', None)
    assert _parse('scaled_gev_atf+mvdr') == ('atf_mvdr', 'scaled_gev_atf', None)
    for f in ('mvdr_souden', 'gev', 'wmwf'):
        assert _parse(f) == ('filter', None, f)
        for r in ('rank1_pca', 'rank1_gev'):
            assert _parse(f'{r}+{f}') == ('filter', r, f)
    for bad in ('nonsense', 'rank1_pca+mvdr', 'gev+mvdr', 'pca+gev', 'chx', 'mvdr', 'rank1_foo+gev'):
        assert _parse(bad)[0] is None, bad


def test_joint_weight_mode_mapping():
    """weight_constant_axis of the joint models (gcacgmm.py:158-162) -> PBBSS_JOINT_WEIGHT_*."""
    from pb_bss_amd import _lib
    from pb_bss_amd.distribution import _joint
    assert _joint.weight_mode((-1,)) == _lib.JOINT_WEIGHT_FK
    assert _joint.weight_mode((2,)) == _lib.JOINT_WEIGHT_FK
    assert _joint.weight_mode((-3, -1)) == _lib.JOINT_WEIGHT_K
    assert _joint.weight_mode((-3,)) == _lib.JOINT_WEIGHT_KT
    # the reference tests `-2 in weight_constant_axis` literally (gcacgmm.py:288)
    assert _joint.weight_mode((-3, -2, -1)) == _lib.JOINT_WEIGHT_UNIFORM
    assert _joint.weight_mode((0, 1, 2)) == _lib.JOINT_WEIGHT_CONST
    assert _joint.weight_mode((-2,)) == _lib.JOINT_WEIGHT_UNIFORM
    assert _joint.weight_mode((-2, -1)) == _lib.JOINT_WEIGHT_UNIFORM


def test_host_samplers_reproduce_reference_draws():
    """sample_cacgmm / ComplexAngularCentralGaussian.sample consume the global NumPy RNG in
    the reference's order (cacgmm.py:27-55, complex_circular_symmetric_gaussian.py:47-69)."""
    import os
    from pb_bss_amd.distribution import ComplexAngularCentralGaussian, sample_cacgmm
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                             'sampler_draws.npz'))
    np.random.seed(11)
    x, labels = sample_cacgmm(50, g['weight'], g['covariance'], return_label=True)
    np.testing.assert_array_equal(labels, g['labels'])
    np.testing.assert_allclose(x, g['x'], atol=1e-12)
    np.testing.assert_allclose(np.linalg.norm(x, axis=-1), 1.0, atol=1e-14)
    np.random.seed(12)
    m = ComplexAngularCentralGaussian(covariance_eigenvectors=g['eigvec'],
                                      covariance_eigenvalues=g['eigval'])
    y = m.sample(size=(20,))
    assert y.shape == (20, 3)
    np.testing.assert_allclose(y, g['y'], atol=1e-12)


def test_transform_windows_match_scipy_and_oracle():
    """Host side of pb_bss_amd.transform: periodic analysis window and the biorthogonal
    synthesis window (the only arithmetic done outside the kernels)."""
    from scipy import signal
    from oracle import stft as o
    from pb_bss_amd.transform import analysis_window, biorthogonal_window, stft_frames_to_samples
    for name, fn in (('blackman', signal.windows.blackman), ('hann', signal.windows.hann),
                     ('hamming', signal.windows.hamming)):
        np.testing.assert_allclose(analysis_window(name, 512), fn(513)[:-1], atol=1e-15)
        np.testing.assert_allclose(analysis_window(name, 400, symmetric_window=True), fn(400),
                                   atol=1e-15)
    np.testing.assert_allclose(analysis_window(signal.windows.blackman, 256),
                               signal.windows.blackman(257)[:-1], atol=0)
    w = analysis_window('blackman', 1024)
    s = biorthogonal_window(w, 256)
    np.testing.assert_allclose(s, o.biorthogonal_window(w, 256), atol=0)
    # defining property: sum_m w[n + m shift] s[n + m shift] == 1
    np.testing.assert_allclose((w * s).reshape(4, 256).sum(0), 1.0, atol=1e-14)
    with pytest.raises(ValueError):
        biorthogonal_window(analysis_window('hann', 400), 128)
    assert stft_frames_to_samples(66, 512, 128) == 66 * 128 + 384 - 768
    assert stft_frames_to_samples(10, 512, 128, fading=False) == 10 * 128 + 384


def test_gmm_and_alignment_argument_mapping():
    """Pure host logic of the GMM / permutation-solver mirrors: how weight_constant_axis,
    covariance_type and similarity_metric map onto the device modes, and the errors the
    reference raises for bad values."""
    from pb_bss_amd.distribution import gmm
    from pb_bss_amd import permutation_alignment as pa
    assert gmm._weight_kind((-1,), 2) == gmm._CLASS
    assert gmm._weight_kind(-1, 3) == gmm._CLASS
    assert gmm._weight_kind([1], 2) == gmm._CLASS       # axis 1 of (K, N) is the sample axis
    assert gmm._weight_kind(-2, 2) == gmm._UNIFORM      # int -2: the constant 1 / K
    assert gmm._weight_kind((-2,), 2) == gmm._ONES      # tuple (-2,): a (1, N) array of ones
    assert gmm._weight_kind((0,), 2) == gmm._ONES
    assert gmm._weight_kind((-3,), 3) is None           # -> the step-wise device loop
    gmm._check_covariance_type('full')
    gmm._check_covariance_type('spherical')
    gmm._check_covariance_type('diagonal')              # served by the step-wise device loop
    with pytest.raises(ValueError, match="Unknown covariance type 'round'"):
        gmm._check_covariance_type('round')
    for metric in ('cos', 'multiply', 'euclidean'):
        pa._check_metric(metric)
        pa.GreedyPermutationAlignment(similarity_metric=metric)
        pa.OraclePermutationAlignment(similarity_metric=metric, algorithm='greedy')
    with pytest.raises(AttributeError, match='Suggestions: cos, euclidean'):
        pa._check_metric('coss')            # getattr(_ScoreMatrix, 'coss') in the reference
    with pytest.raises(ValueError):
        pa.GreedyPermutationAlignment(similarity_metric='coss')
    with pytest.raises(AssertionError):
        pa.OraclePermutationAlignment(algorithm='hungarian')
    # the greedy solver's recursion as a composition of permutations (what the device scans)
    from oracle import permutation_alignment as op
    rng = np.random.default_rng(2)
    K, F = 4, 33
    step = np.stack([rng.permutation(K) for _ in range(F)], 1)
    step[:, 0] = np.arange(K)
    seq = step.copy()
    for f in range(1, F):
        seq[:, f] = seq[seq[:, f - 1], f]       # permutation_alignment.py:698-699
    comp = np.arange(K)
    for f in range(1, F):
        comp = step[comp, f]                    # M_f o (M_{f-1} o ... o M_1)
        assert (comp == seq[:, f]).all()
    assert op.greedy_calculate_mapping(rng.uniform(size=(3, 1, 5))).tolist() == [[0], [1], [2]]


def test_result_dtype_switch_and_rounding_helpers():
    import pb_bss_amd
    from pb_bss_amd.distribution.utils import reference_single, to_single
    y32 = np.zeros(3, np.complex64)
    assert not reference_single(y32)                      # default: working precision
    with pb_bss_amd.result_dtype('reference'):
        assert reference_single(y32, None, np.zeros(2, np.float32))
        assert not reference_single(y32, np.zeros(2))
        assert not reference_single(np.zeros(3, np.complex128))
        with pytest.raises(AssertionError):
            pb_bss_amd.set_result_dtype('float16')
    assert not reference_single(y32)
    assert to_single(None) is None
    assert to_single(np.ones(2)).dtype == np.float32
    assert to_single(np.ones(2, np.complex128)).dtype == np.complex64
    import torch
    assert to_single(torch.ones(2, dtype=torch.complex128)).dtype == torch.complex64


def test_reference_dtype_rounding_of_a_fitted_model():
    """CACGMMTrainer._rounded (result dtype 'reference'): float32 / complex64 fields, the constant
    1/K weight of weight_constant_axis=-2 stays float64, the affiliation of the (model,
    affiliation) form is rounded too; `single=False` passes everything through."""
    from pb_bss_amd import _lib
    from pb_bss_amd.distribution import CACGMM, CACGMMTrainer
    from pb_bss_amd.distribution.complex_angular_central_gaussian import (
        ComplexAngularCentralGaussian)
    F, K, D, T = 2, 3, 4, 5
    rng = np.random.default_rng(0)
    model = CACGMM(
        weight=np.full((F, K, 1), 1 / K),
        cacg=ComplexAngularCentralGaussian(
            covariance_eigenvectors=rng.normal(size=(F, K, D, D)) + 1j * rng.normal(size=(F, K, D, D)),
            covariance_eigenvalues=rng.uniform(size=(F, K, D))))
    aff = rng.uniform(size=(F, K, T))
    assert CACGMMTrainer._rounded(model, False, _lib.WEIGHT_UNIFORM) is model
    m = CACGMMTrainer._rounded(model, True, None)
    assert (m.weight.dtype, m.cacg.covariance_eigenvectors.dtype,
            m.cacg.covariance_eigenvalues.dtype) == (np.float32, np.complex64, np.float32)
    np.testing.assert_allclose(m.cacg.covariance_eigenvalues, model.cacg.covariance_eigenvalues,
                               rtol=1e-6)
    m, a = CACGMMTrainer._rounded((model, aff), True, _lib.WEIGHT_UNIFORM)
    assert m.weight.dtype == np.float64 and a.dtype == np.float32
    assert m.cacg.covariance_eigenvectors.dtype == np.complex64
    assert model.weight.dtype == np.float64                 # the input model is left alone


def test_split_timeout_retry_logic(monkeypatch):
    """engine._checked_with_split_retry without a GPU: the poison pattern plus the flag of
    pbbss_split_error repeats the launch once with the split groups off; the pattern without the
    flag, or any other status, raises the reference's errors; a clean status passes through."""
    import types
    import torch
    from pb_bss_amd import _lib, engine
    dev = types.SimpleNamespace(index=0)
    tails, resets, setting = [], [], [True]
    monkeypatch.setattr(engine, 'set_split_tail', lambda e, d=None: tails.append((bool(e), d)))
    monkeypatch.setattr(engine, 'split_tail', lambda d=None: setting[0])
    monkeypatch.setattr(engine, 'split_reset', lambda d=None: resets.append(d))
    poison = _lib.ST_NONFINITE | _lib.ST_EIG_NOCONV

    def launcher(statuses):
        seq = iter(statuses)
        return lambda: dict(status=torch.tensor(next(seq), dtype=torch.int32), tag=object())

    # clean
    monkeypatch.setattr(engine, 'split_error', lambda d=None: 0)
    r = engine._checked_with_split_retry(launcher([[[0, 0]]]), dev, 'x')
    assert int(r['status'].max()) == 0 and tails == []
    # informational bits alone never raise
    r = engine._checked_with_split_retry(launcher([[[_lib.ST_FLOORED, _lib.ST_SLOWPATH]]]), dev, 'x')
    assert tails == []
    # poison + flag: one repeat without split groups, which are switched on again
    monkeypatch.setattr(engine, 'split_error', lambda d=None: 1)
    with pytest.warns(RuntimeWarning, match='split groups'):
        r = engine._checked_with_split_retry(launcher([[[0, poison]], [[0, 0]]]), dev, 'x')
    assert tails == [(False, 0), (True, 0)] and int(r['status'].max()) == 0
    assert resets == [0]                      # the report was consumed before the repeat
    # a caller who had switched the split groups off gets them back OFF, not on
    tails.clear()
    setting[0] = False
    with pytest.warns(RuntimeWarning, match='split groups'):
        engine._checked_with_split_retry(launcher([[[0, poison]], [[0, 0]]]), dev, 'x')
    assert tails == [(False, 0), (False, 0)]
    setting[0] = True
    # the repeat fails for real: the error is raised, the split groups are on again
    tails.clear()
    with pytest.warns(RuntimeWarning), pytest.raises(AssertionError, match='non-finite'):
        engine._checked_with_split_retry(launcher([[[poison, 0]], [[_lib.ST_NONFINITE, 0]]]), dev, 'x')
    assert tails == [(False, 0), (True, 0)]
    # poison without the flag: a numerical failure as the reference reports it
    tails.clear()
    monkeypatch.setattr(engine, 'split_error', lambda d=None: 0)
    with pytest.raises(AssertionError, match='non-finite'):
        engine._checked_with_split_retry(launcher([[[poison, 0]]]), dev, 'x')
    with pytest.raises(np.linalg.LinAlgError):
        engine._checked_with_split_retry(launcher([[[_lib.ST_EIG_NOCONV, 0]]]), dev, 'x')
    assert tails == []


def test_stack_parameters_nested_models():
    """pb_bss/distribution/utils.py:259-316: nested dataclasses stacked field by field along a new
    leading axis; mixed model types are refused (the doctest's CACGMM(cacg=..., weight=...) shape)."""
    from pb_bss_amd.distribution import CACGMM, ComplexAngularCentralGaussian
    from pb_bss_amd.distribution.utils import stack_parameters
    rng = np.random.default_rng(0)
    models = []
    for _ in range(3):
        cacg = ComplexAngularCentralGaussian(
            covariance_eigenvectors=rng.normal(size=(2, 4, 4)) + 1j * rng.normal(size=(2, 4, 4)),
            covariance_eigenvalues=rng.uniform(size=(2, 4)))
        models.append(CACGMM(weight=rng.uniform(size=(2, 1)), cacg=cacg))
    st = stack_parameters(models)
    assert isinstance(st, CACGMM) and isinstance(st.cacg, ComplexAngularCentralGaussian)
    assert st.weight.shape == (3, 2, 1) and st.cacg.covariance_eigenvectors.shape == (3, 2, 4, 4)
    for i, m in enumerate(models):
        np.testing.assert_array_equal(st.weight[i], m.weight)
        np.testing.assert_array_equal(st.cacg.covariance_eigenvalues[i], m.cacg.covariance_eigenvalues)
    st2 = stack_parameters([m.cacg for m in models])
    np.testing.assert_array_equal(st2.covariance_eigenvectors, st.cacg.covariance_eigenvectors)
    with pytest.raises(AssertionError):
        stack_parameters([models[0], models[0].cacg])
    # torch parameters stay torch
    import torch
    tm = [ComplexAngularCentralGaussian(
        covariance_eigenvectors=torch.from_numpy(m.cacg.covariance_eigenvectors),
        covariance_eigenvalues=torch.from_numpy(m.cacg.covariance_eigenvalues)) for m in models]
    st3 = stack_parameters(tm)
    assert isinstance(st3.covariance_eigenvalues, torch.Tensor)
    np.testing.assert_array_equal(st3.covariance_eigenvalues.numpy(), st2.covariance_eigenvalues)


def test_random_affiliation_consumes_the_reference_stream():
    """`fit(..., num_classes=K)`: the draw comes from NumPy's global generator exactly as in the
    reference (cacgmm.py:205-210) and the device-side normalisation is bit-identical to the
    reference's host expression; the opt-in 'device' draw leaves NumPy's stream untouched."""
    import torch
    from pb_bss_amd.distribution import utils
    np.random.seed(3)
    got = utils.random_affiliation((4, 3, 7), torch.device('cpu')).numpy()
    after = np.random.uniform()
    np.random.seed(3)
    want = np.random.uniform(size=(4, 3, 7))
    want /= np.einsum('...kn->...n', want)[..., None, :]
    assert np.array_equal(got, want) and after == np.random.uniform()
    np.random.seed(5)
    with utils.random_init('device'):
        dev = utils.random_affiliation((2, 3, 5), torch.device('cpu'))
    assert dev.shape == (2, 3, 5) and torch.allclose(dev.sum(-2), torch.ones(2, 5, dtype=torch.float64))
    np.random.seed(5)
    first = np.random.uniform()
    np.random.seed(5)
    utils.set_random_init('device')
    try:
        utils.random_affiliation((2, 3, 5), torch.device('cpu'))
    finally:
        utils.set_random_init('numpy')
    assert np.random.uniform() == first   # the NumPy stream was not consumed


def _bench_modules():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, 'tools')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import bench
    import bench_blocks
    return bench, bench_blocks


def test_committed_profiles_match_the_kernel_sources_of_this_tree():
    """bench.py attaches PMC traffic to its roofline blocks only from a committed rocprofv3 summary
    whose header carries the hash of the kernel sources in the tree: a kernel edit without a new
    profile turns `traffic` into null on the driver's line.  A release check, not a correctness
    check: between a kernel edit and the next profiling run on a GPU it is an expected failure
    (xfail, so the CPU suite stays green and still says which profile is stale)."""
    _, bb = _bench_modules()
    path = bb.matching_profile()
    if path is None:
        pytest.xfail('no profiles/r*_profile.txt carries kernel_source_sha ' + bb.kernel_source_sha() +
                     ': re-run tools/profile_round.sh on this tree')
    prof = bb.read_profile(path)
    assert prof['trace'] is not None and prof['pmc'], path
    stale = []
    for workload in ('config3', 'config4', 'config4_vmf', 'config5'):
        traffic, src = bb.workload_pmc(workload, None)
        if traffic is None or not traffic['bytes_per_step'] > 0:
            stale.append((workload, src))
    if stale:
        pytest.xfail(f'stale workload profiles: {stale}')


def test_bench_line_is_compact_strict_json():
    """The driver parses the LAST stdout line of bench.py; round 5's 27 KB line came back as
    `parsed: null`.  compact_line must turn a full result (canned: the committed round-5 line with
    all five workloads, plus a NaN and an inf planted in it) into strict JSON of at most 8 KB that
    still carries the contract keys, `roofline`, `cpu_baseline` and the per-workload summaries."""
    import json
    import os
    bench, _ = _bench_modules()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'tests', 'golden', 'bench_full_line_r05.json')) as f:
        full = json.load(f)
    full['config5']['roofline']['frac'] = float('nan')
    full['sustained']['value'] = float('inf')
    full['config4']['verify']['mask_max_abs_err'] = np.float64(1e-13)   # numpy scalars happen
    line = bench.compact_line(full, 'gpurun_out/bench_extra.json')
    assert '\n' not in line and len(line.encode()) <= 8192, len(line)

    def no_constants(name):
        raise AssertionError(f'non-strict JSON constant {name}')
    d = json.loads(line, parse_constant=no_constants)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better',
              'scaling', 'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline', 'verify'):
        assert k in d, k
    assert d['value'] == full['value'] and d['ms_per_step'] == full['ms_per_step']
    assert d['config']['workload'].startswith('BASELINE configs[1]')
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'kernel_ms'):
        assert k in d['roofline'], k
    assert d['roofline']['hbm_contract']['frac'] == full['roofline']['hbm_contract']['frac']
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert k in d['cpu_baseline'], k
    assert d['sustained']['value'] is None                      # inf -> null
    assert 'frac' not in d['config5'] and d['config5']['ok'] is True
    assert d['strong']['n_gpus'] == 1 and d['strong']['value'] > 0
    for k in ('f32', 'config3', 'config4', 'config5'):
        assert k in d, k
    assert d['config4']['watson']['mask_err'] == 1e-13 and d['config4']['vmf']['ok'] is True
    # a block that balloons must not push the line over the limit: summaries are dropped first
    full['config3']['single']['unit'] = 'x' * 100
    full['config'] = dict(full['config'], note='y' * 7000)
    line = bench.compact_line(full, None)
    assert len(line.encode()) <= 8192
    d = json.loads(line)
    assert 'roofline' in d and 'cpu_baseline' in d and d['value'] == full['value']


def test_import_surface_of_the_hot_path_modules():
    """A pb_bss user switches the package name and finds every name of the hot-path modules:
    the reference's public functions / classes, module by module (pb_bss/extraction/__init__.py,
    beamformer_wrapper.py, distribution/*.py, permutation_alignment.py, utils.py).  Out of scope
    (SURVEY 2): mask estimators, BinaryGMM, complex Bingham, circular-symmetric Gaussian."""
    import importlib
    want = {
        'extraction': ['get_bf_vector', 'get_single_source_bf_vector', 'get_gev_vector',
                       'get_mvdr_vector_souden', 'get_power_spectral_density_matrix',
                       'blind_analytic_normalization', 'apply_beamforming_vector'],
        'extraction.beamformer_wrapper': [
            'get_bf_vector', 'get_pca_rank_one_estimate', 'get_gev_rank_one_estimate',
            '_get_gev_atf_vector', '_get_atf_vector', '_get_rank_1_approximation',
            '_get_response_vector', 'get_lcmv_vector', 'condition_covariance', 'labels_to_one_hot'],
        'distribution.cacgmm': ['CACGMM', 'CACGMMTrainer', 'log_pdf_to_affiliation',
                                'estimate_mixture_weight', 'normalize_observation'],
        'distribution.cwmm': ['CWMM', 'CWMMTrainer', 'log_pdf_to_affiliation', 'normalize_observation'],
        'distribution.vmfmm': ['VMFMM', 'VMFMMTrainer', 'VonMisesFisherTrainer',
                               'estimate_mixture_weight', 'log_pdf_to_affiliation'],
        'distribution.gmm': ['GMM', 'GMMTrainer', 'GaussianTrainer', 'labels_to_one_hot'],
        'distribution.gcacgmm': [
            'GCACGMM', 'GCACGMMTrainer', 'ComplexAngularCentralGaussianTrainer', 'GaussianTrainer',
            'log_pdf_to_affiliation_for_integration_models_with_inline_pa', 'unsqueeze'],
        'distribution.vmfcacgmm': [
            'VMFCACGMM', 'VMFCACGMMTrainer', 'VonMisesFisherTrainer',
            'log_pdf_to_affiliation_for_integration_models_with_inline_pa', 'unsqueeze'],
        'distribution.complex_angular_central_gaussian': ['force_hermitian', 'is_broadcast_compatible'],
        'distribution.complex_watson': ['ComplexWatson', 'ComplexWatsonTrainer', 'get_pca',
                                        'is_broadcast_compatible'],
        'distribution.mixture_model_utils': [
            'log_pdf_to_affiliation', 'estimate_mixture_weight', 'apply_inline_permutation_alignment',
            'log_pdf_to_affiliation_for_integration_models_with_inline_pa'],
        'distribution.utils': ['force_hermitian', 'get_trainer_class_from_model',
                               'parameter_from_dict', 'stack_parameters'],
        'permutation_alignment': ['DHTVPermutationAlignment', 'OraclePermutationAlignment',
                                  'GreedyPermutationAlignment', 'interleave', 'sample_random_mapping',
                                  'apply_mapping'],
        'utils': ['is_broadcast_compatible', 'labels_to_one_hot', 'unsqueeze', 'get_pca'],
    }
    for mod, names in want.items():
        m = importlib.import_module('pb_bss_amd.' + mod)
        for n in names:
            assert hasattr(m, n), (mod, n)


def test_small_host_helpers_behave_like_the_reference():
    """Doctest values of pb_bss/utils.py:197-345, permutation_alignment.py:11-51,
    distribution/utils.py:6-28, :83-113, :318-329."""
    from pb_bss_amd import utils
    from pb_bss_amd.distribution import ComplexAngularCentralGaussian, utils as du
    from pb_bss_amd.permutation_alignment import interleave, sample_random_mapping
    assert list(interleave([1, 2, 3, 4, 5], list('abcdefg'))) == \
        [1, 'a', 2, 'b', 3, 'c', 4, 'd', 5, 'e', 'f', 'g']
    assert list(interleave(list('abcdefg'), [1, 2, 3, 4, 5])) == \
        ['a', 1, 'b', 2, 'c', 3, 'd', 4, 'e', 5, 'f', 'g']
    assert list(interleave([None, 0], [False])) == [None, False, 0]      # falsy items survive
    rs = np.random.RandomState(3)
    m = sample_random_mapping(4, 9, rs)
    rs = np.random.RandomState(3)
    assert m.shape == (4, 9) and np.array_equal(m, np.stack([rs.permutation(4) for _ in range(9)], 1))
    assert np.array_equal(utils.labels_to_one_hot([0, 1], categories=4),
                          np.array([[1, 0], [0, 1], [0, 0], [0, 0]], dtype=bool))
    hot = utils.labels_to_one_hot([[0, 1], [0, 3]], categories=4, axis=1)
    assert hot.shape == (2, 4, 2) and hot[1, 3, 1] and hot.sum() == 4
    assert utils.labels_to_one_hot(np.array(2), 3, dtype=np.float64).tolist() == [0., 0., 1.]
    assert utils.unsqueeze(np.ones((2, 3)), (-3, -1)).shape == (2, 1, 3, 1)
    assert utils.unsqueeze(13, (-2, -1)).shape == (1, 1)
    with pytest.raises(IndexError):
        utils.unsqueeze(np.ones(2), (5,))
    assert utils.is_broadcast_compatible((2, 3), (3,)) and not utils.is_broadcast_compatible((2, 3), (4, 3))
    A = np.array([[1 + 2j, 3 + 5j], [7 + 11j, 13 + 17j]])
    H = du.force_hermitian(A)
    assert np.allclose(H, [[1, 5 - 3j], [5 + 3j, 13]]) and np.allclose(du.force_hermitian(H), H)
    assert du.get_trainer_class_from_model(ComplexAngularCentralGaussian).__name__ == \
        'ComplexAngularCentralGaussianTrainer'
    assert du.get_trainer_class_from_model(ComplexAngularCentralGaussian()).__name__ == \
        'ComplexAngularCentralGaussianTrainer'
    model = ComplexAngularCentralGaussian(covariance_eigenvectors=np.eye(2)[None],
                                          covariance_eigenvalues=np.ones((1, 2)))
    for cls in ('ComplexAngularCentralGaussian', ComplexAngularCentralGaussian):
        back = du.parameter_from_dict(cls, model.to_dict())
        assert isinstance(back, ComplexAngularCentralGaussian)
        assert np.array_equal(back.covariance_eigenvalues, model.covariance_eigenvalues)


def test_bench_line_survives_a_failed_additional_block():
    """A block beyond the contract that raised (bench.py: guarded) is recorded as {"error": ...}: the
    line keeps the headline, roofline and cpu_baseline and names the failure."""
    import json
    import os
    bench, _ = _bench_modules()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'tests', 'golden', 'bench_full_line_r05.json')) as f:
        full = json.load(f)
    for k in ('f32', 'config3', 'config5', 'single_utterance_chain'):
        full[k] = {'error': 'RuntimeError: out of memory ' * 20}
    full['config4'] = {'error': 'boom', 'vmf': {'error': 'boom too'}}
    line = bench.compact_line(full, None)
    assert len(line.encode()) <= 8192
    d = json.loads(line)
    assert d['value'] == full['value'] and 'roofline' in d and 'cpu_baseline' in d
    assert d['f32']['error'].startswith('RuntimeError') and len(d['f32']['error']) <= 160
    assert d['config3']['error'] and d['config5']['error'] and d['single_utterance_chain']['error']
    assert d['config4'] == {'watson': {'error': 'boom'}, 'vmf': {'error': 'boom too'}}
    assert 'strong' not in d


def test_bench_line_of_a_multi_rank_run_carries_the_strong_curve():
    """The N > 1 line (canned: the full blocks of the N = 2 one-device rehearsal of round 6): the
    top-level `strong` block names the faster sharding of BASELINE configs[2], both shardings' step
    times and the speed-up against the newest committed N = 1 line; `comm` says what the
    collective layer saw; the line stays under the limit."""
    import json
    import os
    bench, _ = _bench_modules()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'tests', 'golden', 'bench_full_line_n2_rehearsal.json')) as f:
        full = json.load(f)
    line = bench.compact_line(full, None)
    assert len(line.encode()) <= 8192
    d = json.loads(line)
    assert d['n_gpus'] == 2 and d['scaling'] == 'weak'
    st = d['strong']
    assert st['n_gpus'] == 2 and st['sharding'] in ('utterances_sharded', 'bins_sharded')
    legs = st['per_sharding_ms_per_step']
    assert set(legs) == {'bins_sharded', 'utterances_sharded'}
    assert st['ms_per_step'] == pytest.approx(min(legs.values()), rel=1e-4)
    assert st['speedup_vs_recorded_n1'] == pytest.approx(
        st['n1_ms_per_step_recorded'] / st['ms_per_step'], rel=1e-4)
    assert d['comm']['world_size'] == 2 and d['comm']['bytes_per_rank'] > 0
    assert d['config3']['mapping_identical_across_shardings'] is True
    assert d['verify']['gathered_masks_identical_on_all_ranks'] is True



def _host_compiler():
    import shutil
    for cxx in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_dispatch_helpers_reach_every_case(tmp_path):
    """csrc/dispatch.hpp turns a runtime value into a template argument for every launch site: each
    value of a range reaches the lambda with its constant, values outside return
    PBBSS_ERR_UNSUPPORTED without a call, the lambda's status is passed through.  Host-only C++17
    (tests/cpp/dispatch_check.cpp), built with the host compiler: the header includes no HIP."""
    import subprocess
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / 'dispatch_check'
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Wextra', '-Werror', '-O1',
                    '-I', os.path.join(root, 'pb_bss_amd', 'csrc'), '-I', os.path.join(root, 'include'),
                    os.path.join(root, 'tests', 'cpp', 'dispatch_check.cpp'), '-o', str(exe)],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


def test_dynamic_lds_attribute_is_set_in_one_function():
    """hipFuncAttributeMaxDynamicSharedMemorySize belongs to a function on a device, shared by all
    host threads: it may only be raised.  raise_lds_attribute (csrc/launch_util.hpp) keeps that
    invariant; no launch site sets the attribute itself."""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    token = 'hipFuncAttributeMaxDynamicSharedMemorySize'
    users = {}
    for path in sorted(glob.glob(os.path.join(root, 'pb_bss_amd', 'csrc', '*.h*'))):
        with open(path) as f:
            text = f.read()
        if token in text:
            users[os.path.basename(path)] = text
    assert list(users) == ['launch_util.hpp'], list(users)
    text = users['launch_util.hpp']
    start = text.index('inline bool raise_lds_attribute(const void* fn')
    depth, end = 0, None
    for i in range(text.index('{', start), len(text)):
        depth += {'{': 1, '}': -1}.get(text[i], 0)
        if depth == 0:
            end = i
            break
    assert end is not None
    assert token not in text[:start] and token not in text[end:]
    assert text[start:end].count('hipFuncSetAttribute(fn,') == text.count('hipFuncSetAttribute(fn,') > 0
