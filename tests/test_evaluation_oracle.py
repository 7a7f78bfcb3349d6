"""CPU: the import surface of pb_bss_amd.evaluation, and the float64 restatement of the
reference's metrics (tests/oracle_evaluation.py) against the reference's recorded results
(tests/golden/evaluation.npz) and against the live reference."""
import inspect
import os

import numpy as np
import pytest

import oracle_evaluation as oe

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evaluation.npz')
# restatement vs reference: the same float64 operations in the same order (the issue measured
# 7e-15 dB between two orderings); values of at most a few ten dB
TOL = 1e-12

DOC_VALUES = [np.inf, np.inf, -25.127672346460717, 0.481070445785553, 6.3704606032577304,
              6.3704606032577304]


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case(golden, name):
    return {k.split('/', 1)[1]: v for k, v in golden.items() if k.split('/', 1)[0] == name}


def names(golden, prefix):
    return sorted({k.split('/', 1)[0] for k in golden if k.startswith(prefix)})


def assert_close(got, want, tol=TOL):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    finite = np.isfinite(want)
    np.testing.assert_array_equal(got[~finite], want[~finite])
    if finite.any():
        assert np.abs(got[finite] - want[finite]).max() <= tol


def doc_pairs(reference):
    return [(reference, reference), (reference, reference * 2), (reference, np.flip(reference)),
            (reference, reference + np.flip(reference)), (reference, reference + 0.5),
            (reference, reference * 2 + 1)]


def test_import_surface():
    """fails without the evaluation package"""
    import pb_bss_amd.evaluation as ev
    from pb_bss_amd import _lib
    from pb_bss_amd.evaluation import module_si_sdr, si_sdr, sxr_module
    assert ev.si_sdr is module_si_sdr.si_sdr is si_sdr
    assert ev.sxr_module is sxr_module
    assert sxr_module.__all__ == oe.SXR_NAMES
    for name in oe.SXR_NAMES + ['set_snr']:
        assert callable(getattr(sxr_module, name)), name
    assert sxr_module.ResultTuple.__name__ == 'SXR'
    assert sxr_module.ResultTuple._fields == ('sdr', 'sir', 'snr')
    assert list(inspect.signature(si_sdr).parameters) == ['reference', 'estimation']
    sig = inspect.signature(sxr_module.get_snr)
    assert list(sig.parameters) == ['X', 'N', 'axis', 'keepdims']
    assert sig.parameters['axis'].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(sxr_module.set_snr)
    assert list(sig.parameters) == ['X', 'N', 'snr', 'current_snr', 'axis', 'inplace']
    assert sig.parameters['inplace'].default is True
    sig = inspect.signature(sxr_module.input_sxr)
    assert list(sig.parameters) == ['images', 'noise', 'average_sources', 'average_channels',
                                    'return_dict']
    assert sig.parameters['return_dict'].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(sxr_module.output_sxr)
    assert list(sig.parameters) == ['image_contribution', 'noise_contribution',
                                    'average_sources', 'return_dict', 'return_selection']
    assert sig.parameters['return_dict'].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert sig.parameters['return_selection'].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters['return_selection'].default is False
    assert isinstance(module_si_sdr.SPAN, int) and module_si_sdr.SPAN % 4 == 0
    for export in ('pbbss_signal_power', 'pbbss_si_sdr', 'pbbss_output_sxr', 'pbbss_input_sxr'):
        assert export in _lib.EXPORTS and hasattr(_lib.load(), export)


def test_python_constants_match_the_kernels():
    """the span the GPU tests take their edge lengths from, and the bounds the host layer checks
    before it calls, are the values csrc/eval.hpp compiles into the kernels"""
    import re
    from pb_bss_amd.evaluation import module_si_sdr, sxr_module
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'pb_bss_amd', 'csrc', 'eval.hpp')) as f:
        text = f.read()

    def constant(name):
        found = re.findall(r'constexpr int ' + name + r' = (\d+);', text)
        assert len(found) == 1, name
        return int(found[0])

    assert module_si_sdr.SPAN == constant('kEvalSpan')
    assert module_si_sdr._MAX_ROWS == constant('kEvalMaxRows')
    assert sxr_module._MAX_TARGETS == constant('kSxrMaxTargets')
    assert constant('kSxrMaxSources') == 9 and constant('kSxrMaxSensors') == 29  # K < 10, D < 30


@pytest.mark.needs_reference
def test_signatures_match_reference():
    from pb_bss_amd.evaluation import module_si_sdr, sxr_module
    ref_si, ref_sxr = oe.load_reference()
    assert sxr_module.__all__ == ref_sxr.__all__
    assert sxr_module.ResultTuple._fields == ref_sxr.ResultTuple._fields
    pairs = [(module_si_sdr.si_sdr, ref_si.si_sdr)]
    pairs += [(getattr(sxr_module, n), getattr(ref_sxr, n))
              for n in ref_sxr.__all__ + ['set_snr']]
    for ours, theirs in pairs:
        a, b = inspect.signature(ours), inspect.signature(theirs)
        extra = ['return_selection'] if ours.__name__ == 'output_sxr' else []
        assert list(a.parameters) == list(b.parameters) + extra, ours.__name__
        for p in b.parameters:
            assert a.parameters[p].default == b.parameters[p].default, (ours.__name__, p)
            assert a.parameters[p].kind == b.parameters[p].kind, (ours.__name__, p)


def test_refusals_need_no_gpu():
    """argument checks come before the device is touched"""
    from pb_bss_amd.evaluation import si_sdr, sxr_module
    with pytest.raises(AssertionError):
        si_sdr(np.zeros(4, np.float32), np.zeros(4, np.float32))  # the reference's float64 assert
    with pytest.raises(AssertionError):
        si_sdr(np.zeros(4), np.zeros(4, np.int64))
    z = np.zeros
    with pytest.raises(AssertionError):
        sxr_module.output_sxr(z((2, 3, 10)), z((2, 10)))    # noise shape
    with pytest.raises(AssertionError):
        sxr_module.output_sxr(z((10, 10, 4)), z((10, 4)))   # K < 10
    with pytest.raises(AssertionError):
        sxr_module.output_sxr(z((3, 2, 10)), z((2, 10)))    # more sources than outputs
    with pytest.raises(NotImplementedError, match='at most 8'):
        sxr_module.output_sxr(z((2, 9, 10)), z((9, 10)))
    with pytest.raises(AssertionError):
        sxr_module.input_sxr(z((2, 3, 10)), z((4, 10)))     # noise shape
    with pytest.raises(AssertionError):
        sxr_module.input_sxr(z((10, 3, 10)), z((3, 10)))    # K < 10
    with pytest.raises(AssertionError):
        sxr_module.input_sxr(z((2, 30, 10)), z((30, 10)))   # D < 30


def test_si_sdr_docstring_values(golden):
    c = case(golden, 'si_sdr_doc')
    np.random.seed(0)
    reference = np.random.randn(100)
    np.testing.assert_array_equal(reference, c['reference'])
    got = np.array([oe.si_sdr(r, e) for r, e in doc_pairs(reference)])
    assert_close(got, np.array(DOC_VALUES))
    assert_close(got, c['results'])
    assert np.isnan(oe.si_sdr([1., 0], [0., 0])) and np.isnan(c['zero_estimate'])
    assert np.isnan(oe.si_sdr([0., 0], [1., 0]))
    two = oe.si_sdr([reference, reference], [reference * 2 + 1, reference * 1 + 0.5])
    assert_close(two, c['two_rows'])
    assert_close(two, np.array([6.3704606032577304, 6.3704606032577304]))


def test_si_sdr_restatement_equals_recorded(golden):
    for name in ('si_sdr_rows', 'si_sdr_outer'):
        c = case(golden, name)
        assert_close(oe.si_sdr(c['reference'], c['estimation']), c['result'])
    assert case(golden, 'si_sdr_outer')['result'].shape == (2, 3)


def test_get_snr(golden):
    assert oe.get_snr([1, 2, 3], [1, 2, 3]) == 0.0
    for name in ('get_snr_real', 'get_snr_complex'):
        c = case(golden, name)
        assert_close(oe.get_snr(c['X'], c['N']), c['all'])
        assert_close(oe.get_snr(c['X'], c['N'], axis=-1), c['last'])
        assert_close(oe.get_snr(c['X'], c['N'], axis=(0, 2)), c['pair'])
        assert_close(oe.get_snr(c['X'], c['N'], axis=1, keepdims=True), c['keepdims'])
        assert c['keepdims'].shape == (3, 1, 100)


def test_input_sxr_restatement_equals_recorded(golden):
    cases = names(golden, 'input_sxr_')
    assert len(cases) == 3
    for name in cases:
        c = case(golden, name)
        for sources in (True, False):
            for channels in (True, False):
                got = oe.input_sxr(c['images'], c['noise'], sources, channels)
                assert_close(np.stack(got), c[f'result_{int(sources)}{int(channels)}'])
    assert np.all(np.isposinf(case(golden, 'input_sxr_1_2')['result_00'][1]))  # K = 1: SIR


def test_output_sxr_restatement_equals_recorded(golden):
    cases = names(golden, 'output_sxr_')
    assert len(cases) == 9
    for name in cases:
        c = case(golden, name)
        for sources in (True, False):
            details = {}
            got, sel = oe.output_sxr(c['contribution'], c['noise'], sources, details)
            assert_close(np.stack(got), c[f'result_{int(sources)}'])
            assert details['margin'] >= oe.MARGIN, (name, details)
            assert len(set(sel.tolist())) == sel.size
    assert np.all(np.isposinf(case(golden, 'output_sxr_1_2')['result_0'][1]))  # Ks = 1: SIR


def test_output_sxr_batch_and_selection():
    """the batch axes are a loop over the items, and the items of a batch pick differently"""
    co, no = oe.gen_output_case(0, (5,), 3, 3, 200)
    details = {}
    got, sel = oe.output_sxr(co, no, False, details)
    assert sel.shape == (5, 3) and got.sdr.shape == (5, 3)
    assert len({tuple(s) for s in sel.tolist()}) > 1
    assert details['margin'].min() >= oe.MARGIN
    for b in range(5):
        one, sel_one = oe.output_sxr(co[b], no[b], False)
        np.testing.assert_array_equal(np.stack(one), np.stack(got)[:, b])
        np.testing.assert_array_equal(sel_one, sel[b])


@pytest.mark.needs_reference
def test_restatement_equals_live_reference():
    ref_si, ref_sxr = oe.load_reference()
    r, e = oe.gen_si_sdr(5, (4, 777))
    assert_close(oe.si_sdr(r, e), ref_si.si_sdr(r, e))
    assert_close(oe.si_sdr(r[:, None], e[None]), ref_si.si_sdr(r[:, None], e[None]))
    X, N = oe.gen_signals(6, (2, 5, 64), np.complex128), oe.gen_signals(7, (2, 5, 64))
    assert_close(oe.get_snr(X, N, axis=(0, 2)), ref_sxr.get_snr(X, N, axis=(0, 2)))
    for seed in range(4):
        co, no = oe.gen_output_case(seed, (), 3, 4, 500)
        for sources in (True, False):
            got, _ = oe.output_sxr(co, no, sources)
            assert_close(np.stack(got), np.stack(ref_sxr.output_sxr(co, no, sources)))
        im, no = oe.gen_input_case(seed, (), 3, 4, 500)
        for sources in (True, False):
            for channels in (True, False):
                got = oe.input_sxr(im, no, sources, channels)
                assert_close(np.stack(got), np.stack(ref_sxr.input_sxr(im, no, sources, channels)))
    # the reference returns the tuple for a str prefix of output_sxr, a dict for input_sxr
    assert isinstance(ref_sxr.output_sxr(co, no, True, 'out_'), tuple)
    assert sorted(ref_sxr.input_sxr(im, no, return_dict='in_')) == ['in_sdr', 'in_sir', 'in_snr']
