"""CPU: the interface of `evaluation.stoi`, and the float64 restatement of tests/oracle_stoi.py
against the eight STOI values the reference's tests/test_evaluation/test_wrapper_values.py
records of the `pystoi` package (at the reference's own tolerances: 1e-5 relative for the input
metrics, 1e-6 for the output metrics; the restatement sits at 1.2e-6 and 3.4e-7, the rounding of
the recorded digits), its resampler against scipy.signal.resample_poly, and the conditions the
bound of tests/test_gpu_stoi.py is stated for.
"""
import inspect
import os
import re

import numpy as np
import pytest

import oracle_stoi as ost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ['pbbss_resample_poly', 'pbbss_stoi']
RATES = (8000, 12000, 16000, 44100)


def parameters(function):
    return [(p.name, p.default, p.kind) for p in inspect.signature(function).parameters.values()]


def test_import_surface():
    from pb_bss_amd import evaluation
    from pb_bss_amd.evaluation import module_stoi
    assert 'stoi' in evaluation.__all__ and evaluation.stoi is module_stoi.stoi
    empty = inspect.Parameter.empty
    kind = inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert parameters(module_stoi.stoi) == [
        ('reference', empty, kind), ('estimation', empty, kind), ('sample_rate', empty, kind)]
    # the window the module uploads is the restatement's
    for rate in RATES:
        up, down = ost.resample_ratio(rate)
        np.testing.assert_array_equal(module_stoi.resample_window(up, down),
                                      ost.resample_window(up, down))


@pytest.mark.needs_reference
def test_signature_equals_the_reference():
    from pb_bss_amd.evaluation import module_stoi
    assert parameters(module_stoi.stoi) == parameters(ost.load_reference_stoi())


def test_exports_in_header_and_binding():
    from pb_bss_amd import _lib
    with open(os.path.join(ROOT, 'include', 'pbbss.h')) as f:
        header = f.read()
    for name in EXPORTS:
        assert re.search(r'\bint ' + name + r'\s*\(', header), name
        assert name in _lib.SIGNATURES and name in _lib.EXPORTS
    with open(os.path.join(ROOT, 'pb_bss_amd', 'csrc', 'Makefile')) as f:
        makefile = f.read()
    assert '$(BUILD)/stoi.o' in makefile and '$(BUILD)/capi_stoi.o' in makefile


@pytest.mark.needs_reference
def test_restatement_matches_the_recorded_values():
    pytest.importorskip('scipy.signal')  # the reference's scenario convolves with it
    example = ost.load_reference_scenario()()
    source, observation = example['speech_source'], example['observation']
    # InputMetrics.stoi: every source against every channel of the observation
    got = ost.stoi(source[:, None, :], observation[None, :, :], 8000)
    error = np.max(np.abs(got / np.array(ost.RECORDED_INPUT) - 1))
    print(f'input metrics: relative {error:.2e}')
    np.testing.assert_allclose(got, ost.RECORDED_INPUT, rtol=ost.RECORDED_INPUT_RTOL)
    # OutputMetrics.stoi: image plus noise at the first channel as the prediction
    prediction = example['speech_image'][..., 0, :] + example['noise_image'][..., 0, :]
    got = ost.stoi(source, prediction, 8000)
    error = np.max(np.abs(got / np.array(ost.RECORDED_OUTPUT) - 1))
    print(f'output metrics: relative {error:.2e}')
    np.testing.assert_allclose(got, ost.RECORDED_OUTPUT, rtol=ost.RECORDED_OUTPUT_RTOL)


@pytest.mark.parametrize('rate', RATES)
def test_direct_sum_resampler_matches_scipy(rate):
    signal = pytest.importorskip('scipy.signal')
    up, down = ost.resample_ratio(rate)
    window = ost.resample_window(up, down)
    assert (len(window) - 1) // 2 == {8000: 182, 12000: 218, 16000: 290, 44100: 15973}[rate]
    for N in (1, 7, 300, 3001):
        x = np.random.default_rng(N).standard_normal(N)
        got = ost.resample_poly(x, up, down, window)
        want = signal.resample_poly(x, up, down, window=window)
        assert got.shape == want.shape == (-(-N * up // down),)
        assert np.max(np.abs(got - want)) <= 1e-13, (rate, N)


def test_band_edges():
    edges = ost.band_edges()
    assert edges[0].tolist() == [7, 9] and edges[-1].tolist() == [174, 219]
    assert (edges[1:, 0] == edges[:-1, 1]).all()  # neighbours share their edge (csrc/stoi.hip)


def test_cases_are_what_they_are_for():
    """the frame counts the cases of the device test are chosen for"""
    frames = {name: ost.stoi_10k(x, y, details=True) for name, (x, y) in ost.cases_10k().items()}
    assert frames['n4096'] == (ost.SHORT, (30, 30))  # 29 STFT frames
    assert frames['n4097'][1] == (31, 31) and frames['n4097'][0] != ost.SHORT  # one segment
    assert frames['n4224'][1] == (31, 31) and frames['n4225'][1] == (32, 32)
    assert frames['short'] == (ost.SHORT, (0, 0))
    assert frames['sparse'][1] == (155, 31) and frames['sparse'][0] != ost.SHORT
    before, after = frames['long'][1]
    assert before == 1170 > 4 * 256 and after < before
    assert (after - 1 - 29) * ost.BANDS > 64 * 256  # (segment, band) items: more than 64 workgroups
    x, _ = ost.cases_10k()['gaps']
    energies = ost.frame_energies(x)
    keep = (energies.max() - ost.DYN_RANGE - energies) < 0
    assert not keep[0] and not keep[-1] and frames['gaps'][1] == (92, int(keep.sum()))
    # one kept frame whose two neighbours are removed
    assert any(keep[f] and not keep[f - 1] and not keep[f + 1] for f in range(1, len(keep) - 1))


def test_conditions_of_the_device_bound():
    """every frame energy at least 1e-6 dB from the threshold (a rounding difference cannot flip
    a frame) and every reference segment band with a centred norm above 1e-6 of its norm"""
    pairs = [(name, x, y, ost.FS) for name, (x, y) in ost.cases_10k().items()]
    for rate, N in ((8000, 5000), (16000, 8000), (ost.FS, 6000)):
        reference, estimation = ost.gen_matrix(7, N)
        pairs += [(f'matrix{rate}/{k}', reference[k, 0], estimation[0, 0], rate)
                  for k in range(reference.shape[0])]
        a, b = ost.gen_mixed_rows(11, N)
        pairs += [(f'mixed{rate}/{k}', a[k], b[k], rate) for k in range(len(a))]
    for name, x, y, rate in pairs:
        margin, ratio = ost.conditions(x, y, rate)
        print(f'{name}: {margin:.3g} dB from the threshold, centred / plain norm {ratio:.3g}')
        assert margin >= 1e-6, name
        assert ratio > 1e-6, name
