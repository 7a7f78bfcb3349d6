"""CPU: the BSS-Eval yardstick (tests/oracle_bss_eval.py) against the recorded answer of the real
package and against itself, the conditions the GPU bound is stated for, and the public interface
of pb_bss_amd.evaluation against the reference's."""
import inspect

import numpy as np
import pytest

import oracle_bss_eval as ob

# (K, Ke, N, L) of the GPU parity cases (tests/test_gpu_bss_eval.py) that are generated; the
# span cases use the same generator with N around the correlation span
CASES = [
    (1, 1, 40, 4),
    (2, 2, 1000, 8),
    (3, 3, 1500, 24),
    (3, 4, 1500, 24),
    (3, 3, 2000, 64),
    (2, 2, 2047, 16),
    (2, 2, 2049, 16),
    (2, 2, 4097, 16),
    (5, 6, 1200, 4),  # 720 candidate selections: more than one per lane of the search
]
BIG_CASE = (2, 2, 16000, 512)


def case_seed(K, Ke, N, L):
    if (K, Ke, N, L) == BIG_CASE:
        return 5  # among the first seeds, one whose cond(G) is below the 1e3 the bound assumes
    return 1000 * K + 100 * Ke + N + L


@pytest.fixture(scope='module')
def doctest_normal():
    source, prediction = ob.doctest_signals()
    details = {}
    out = ob.bss_eval(source, prediction, route='normal', details=details)
    return out, details


def test_normal_route_reproduces_recorded_doctest(doctest_normal):
    (sdr, sir, sar, selection), _ = doctest_normal
    for name, value in zip(('sdr', 'sir', 'sar'), (sdr, sir, sar)):
        err = np.abs(value - ob.DOCTEST[name]).max()
        print(name, value, err)
        assert err < 1e-4, (name, value)
    assert selection.tolist() == ob.DOCTEST['selection'].tolist()


def channel_case(K, Ke, D, N):
    """(K, D, N) against (Ke, D, N): an independent generated problem per channel"""
    pairs = [ob.gen_case(50 + d, K, Ke, N) for d in range(D)]
    return np.stack([p[0] for p in pairs], axis=1), np.stack([p[1] for p in pairs], axis=1)


def shared_case(seed, K, Ke, D, N):
    """references (K, N) and estimations (Ke, D, N): every channel its own diagonally dominant
    mix (1 on the diagonal, U(0.1, 0.3) off it, plus 0.1 * white noise) of the same references"""
    rng = np.random.default_rng(seed)
    references = ob.ar1(rng, K, N)
    mix = rng.uniform(0.1, 0.3, (D, Ke, K))
    mix[:, np.arange(K), np.arange(K)] = 1.0
    estimations = np.einsum('dek,kn->edn', mix, references) \
        + 0.1 * rng.standard_normal((Ke, D, N))
    return references, estimations


def input_metrics_case():
    """the references of BIG_CASE and an observation (D = 2, N) that mixes them"""
    K, Ke, N, L = BIG_CASE
    references = ob.gen_case(case_seed(*BIG_CASE), K, Ke, N)[0]
    rng = np.random.default_rng(22)
    observation = rng.uniform(0.5, 1.0, (2, K)) @ references + 0.1 * rng.standard_normal((2, N))
    return references, observation


def _per_channel(references, estimations, L):
    if references.ndim == 2:
        references = np.repeat(references[:, None], estimations.shape[1], axis=1)
    return [(references[:, d], estimations[:, d], L, True) for d in range(estimations.shape[1])]


# Every generated input the GPU tests hold to the 1e-9 dB bound, as a list of problems
# (references (K, N), estimations (Ke, N), L, is the selection searched).  InputMetrics scores
# every channel of the observation against every source: its channels are the estimates here.
GENERATED = {str(shape): (lambda shape=shape: [ob.gen_case(case_seed(*shape), *shape[:3])
                                               + (shape[3], True)])
             for shape in CASES + [BIG_CASE]}
GENERATED.update({
    'float32 input': lambda: [tuple(x.astype(np.float64) for x in ob.gen_case(
        case_seed(3, 3, 1500, 24), 3, 3, 1500, dtype=np.float32)) + (24, True)],
    'channel batch': lambda: _per_channel(*channel_case(2, 3, 3, 700), 12),
    'shared references': lambda: _per_channel(*shared_case(11, 2, 2, 3, 900), 16),
    'InputMetrics': lambda: [input_metrics_case() + (BIG_CASE[3], False)],
})


@pytest.mark.parametrize('name', list(GENERATED))
def test_routes_agree_and_conditions_hold(name):
    for references, estimations, L, searched in GENERATED[name]():
        d_direct, d_normal = {}, {}
        direct = ob.bss_eval(references, estimations, L, route='direct', details=d_direct)
        normal = ob.bss_eval(references, estimations, L, route='normal', details=d_normal)
        diff = ob.table_difference(d_direct['tables'], d_normal['tables'])
        cond = ob.gram_condition(references, L)
        finite = d_direct['tables'][np.isfinite(d_direct['tables'])]
        print(name, 'routes differ by', diff, 'cond', cond, 'margin', d_direct['margin'],
              'range', finite.min(), finite.max())
        assert diff < 1e-11
        # the conditions the 1e-9 dB bound of the GPU tests is stated for
        assert cond <= 1e3
        assert np.abs(finite).max() <= 40  # K = 1 has no interference: its SIR is inf
        if searched:
            assert direct[3].tolist() == normal[3].tolist()
            assert d_direct['margin'] >= 1e-3


def test_dependent_references_are_singular_and_routes_agree():
    references, estimations = ob.gen_dependent_case(7)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(ob.correlations(references, estimations[0], 24)[0])
    direct = ob.bss_eval(references, estimations, 24, route='direct')
    normal = ob.bss_eval(references, estimations, 24, route='normal')
    for a, b in zip(direct[:3], normal[:3]):
        assert np.abs(a - b).max() < 1e-6
    assert direct[3].tolist() == normal[3].tolist()


@pytest.mark.needs_reference
def test_signatures_equal_the_reference():
    from pb_bss_amd.evaluation import module_mir_eval, wrapper
    ref_mir_eval, ref_wrapper = ob.load_reference()
    ours = inspect.signature(module_mir_eval.mir_eval_sources)
    assert 'filter_length' in ours.parameters
    assert ours.parameters['filter_length'].kind is inspect.Parameter.KEYWORD_ONLY
    without = ours.replace(parameters=[p for name, p in ours.parameters.items()
                                       if name != 'filter_length'])
    assert without == inspect.signature(ref_mir_eval.mir_eval_sources)
    for name in ('InputMetrics', 'OutputMetrics'):
        assert inspect.signature(getattr(wrapper, name).__init__) == \
            inspect.signature(getattr(ref_wrapper, name).__init__), name


def test_public_names():
    import pb_bss_amd.evaluation as evaluation
    for name in ('mir_eval_sources', 'InputMetrics', 'OutputMetrics'):
        assert name in evaluation.__all__
        assert hasattr(evaluation, name)
    assert evaluation.InputMetrics.__init__.__defaults__ == (None, None, None, False)


def test_unavailable_metrics_are_disabled_not_available():
    from pb_bss_amd.evaluation import OutputMetrics, InputMetrics
    source, prediction = ob.doctest_signals()
    for metrics in (OutputMetrics(prediction, source), InputMetrics(prediction, source)):
        for name in ('pesq', 'stoi', 'srmr'):
            assert name not in metrics._available_metric_names()
            assert name in metrics._disabled_metric_names()
            with pytest.raises(NotImplementedError, match='package'):
                metrics[name]
        with pytest.raises(KeyError, match='Close matches'):
            metrics['mir_eval_sdx']
        with pytest.raises(ValueError, match='enable_si_sdr'):
            metrics.si_sdr
    assert 'mir_eval_selection' in OutputMetrics(prediction, source)._available_metric_names()
