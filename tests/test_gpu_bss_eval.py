"""GPU: pb_bss_amd.evaluation.mir_eval_sources, InputMetrics and OutputMetrics against the float64
yardstick of tests/oracle_bss_eval.py (its direct route: the explicit delay matrix and lstsq).

Bound of the parity cases: 1e-9 dB, the bound tests/test_gpu_evaluation.py asserts for dB
values.  The generated cases have cond(G) <= 1e3 and K L <= 1024 (tests/test_bss_eval_oracle.py
asserts it): a backward-stable solve perturbs the projection by about n cond 2^-53 ~ 1e-10
relative, and with the residuals formed explicitly that is what reaches the energies.  The two
cases that take the host fallback (singular normal equations: the filters are not unique, only
the projection is) are held to 1e-6 dB.
"""
import functools

import numpy as np
import pytest

import oracle_bss_eval as ob
from test_bss_eval_oracle import (BIG_CASE, CASES, case_seed, channel_case, input_metrics_case,
                                  shared_case)

pytestmark = pytest.mark.gpu

BOUND = 1e-9
FALLBACK_BOUND = 1e-6


@functools.lru_cache(maxsize=None)
def generated(shape, compute_permutation=True):
    K, Ke, N, L = shape
    references, estimations = ob.gen_case(case_seed(*shape), K, Ke, N)
    details = {}
    expected = ob.bss_eval(references, estimations, L, compute_permutation, 'direct', details)
    return references, estimations, expected, details


def evaluate(references, estimations, L, compute_permutation=True):
    """-> (sdr, sir, sar, selection) as NumPy (K,), tables (3, Ke, K), status word"""
    from pb_bss_amd import _lib
    from pb_bss_amd.evaluation import module_mir_eval
    info = {}
    values, selection, *_ = module_mir_eval._evaluate(references, estimations,
                                                      compute_permutation, L, info)
    values, selection = _lib.to_host(values), _lib.to_host(selection)
    assert values.shape[1] == 1
    return (values[0, 0], values[1, 0], values[2, 0], selection[0]), \
        _lib.to_host(info['tables'])[0], int(info['status'][0])


def largest_difference(got, expected):
    return max(ob.table_difference(g, e) for g, e in zip(got[:3], expected[:3]))


def test_span_constant_matches_the_cases():
    from pb_bss_amd.evaluation import module_mir_eval
    span = module_mir_eval.SPAN
    assert {(2, 2, span - 1, 16), (2, 2, span + 1, 16), (2, 2, 2 * span + 1, 16)} <= set(CASES)


@pytest.mark.parametrize('shape', CASES + [BIG_CASE])
def test_parity(shape):
    L = shape[3]
    references, estimations, expected, details = generated(shape)
    got, tables, status = evaluate(references, estimations, L)
    diff_tables = ob.table_difference(tables, details['tables'])
    diff = largest_difference(got, expected)
    print(f'{shape}: largest difference {max(diff, diff_tables):.3e} dB, status {status}')
    assert status == 0
    assert got[3].tolist() == expected[3].tolist()
    assert diff_tables < BOUND
    assert diff < BOUND


def test_float32_input():
    from pb_bss_amd.evaluation import mir_eval_sources
    shape = (3, 3, 1500, 24)
    references, estimations = ob.gen_case(case_seed(*shape), 3, 3, 1500, dtype=np.float32)
    expected = ob.bss_eval(references.astype(np.float64), estimations.astype(np.float64), 24)
    got = mir_eval_sources(references, estimations, filter_length=24)
    diff = largest_difference(got, expected)
    print(f'float32 {shape}: largest difference {diff:.3e} dB')
    assert all(v.dtype == np.float64 for v in got[:3])
    assert got[3].tolist() == expected[3].tolist()
    assert diff < BOUND


def test_channel_batch():
    from pb_bss_amd.evaluation import mir_eval_sources
    references, estimations = channel_case(2, 3, 3, 700)
    expected = ob.bss_eval_channels(references, estimations, 12)
    got = mir_eval_sources(references, estimations, filter_length=12)
    assert all(g.shape == (2, 3) for g in got)
    diff = largest_difference(got, expected)
    print(f'(K=2, Ke=3, D=3, N=700, L=12): largest difference {diff:.3e} dB')
    assert got[3].dtype == np.int64 and got[3].tolist() == expected[3].tolist()
    assert diff < BOUND


def test_without_permutation_and_return_dict():
    from pb_bss_amd.evaluation import mir_eval_sources
    shape = (3, 3, 1500, 24)
    references, estimations, expected, _ = generated(shape, False)
    got = mir_eval_sources(references, estimations, compute_permutation=False, filter_length=24)
    assert len(got) == 3
    diff = largest_difference(got, expected)
    print(f'{shape} without the search: largest difference {diff:.3e} dB')
    assert diff < BOUND
    as_dict = mir_eval_sources(references, estimations, return_dict=True,
                               compute_permutation=False, filter_length=24)
    assert sorted(as_dict) == ['sar', 'sdr', 'sir']
    assert all(np.array_equal(as_dict[name], value) for name, value in zip(('sdr', 'sir', 'sar'),
                                                                         got))
    with_search = mir_eval_sources(references, estimations, return_dict=True, filter_length=24)
    assert sorted(with_search) == ['sar', 'sdr', 'selection', 'sir']
    assert with_search['selection'].tolist() == generated(shape)[2][3].tolist()


def test_shared_references_device_tensors_and_repeatability():
    import torch
    from pb_bss_amd.evaluation import mir_eval_sources
    K, D, N, L = 2, 3, 900, 16
    references, estimations = shared_case(11, K, K, D, N)
    ref = torch.from_numpy(references).cuda()
    est = torch.from_numpy(estimations).cuda()
    shared = ref[:, None, :].expand(K, D, N)
    assert shared.stride(1) == 0
    first = mir_eval_sources(shared, est, filter_length=L)
    copied = mir_eval_sources(shared.contiguous(), est, filter_length=L)
    again = mir_eval_sources(shared, est, filter_length=L)
    for a, b, c in zip(first, copied, again):
        assert a.is_cuda and a.shape == (K, D)
        assert torch.equal(a, b)  # bit-identical
        assert torch.equal(a, c)
    assert all(v.dtype == torch.float64 for v in first[:3]) and first[3].dtype == torch.int64
    expected = ob.bss_eval_channels(np.repeat(references[:, None], D, axis=1), estimations, L)
    diff = largest_difference([v.cpu().numpy() for v in first], expected)
    print(f'shared references (K=2, D=3, N=900, L=16): largest difference {diff:.3e} dB')
    assert diff < BOUND
    assert first[3].cpu().numpy().tolist() == expected[3].tolist()


def test_more_items_than_one_launch_set():
    """33 000 items run as two groups; three distinct items repeated, so every item has to
    carry the bits the three give on their own"""
    import torch
    from pb_bss_amd.evaluation import mir_eval_sources
    K, D, N, L, copies = 1, 3, 40, 4, 11000
    references, estimations = channel_case(K, K, D, N)
    ref = torch.from_numpy(references).cuda()
    est = torch.from_numpy(estimations).cuda()
    few = mir_eval_sources(ref, est, filter_length=L)
    many = mir_eval_sources(ref.repeat(1, copies, 1), est.repeat(1, copies, 1), filter_length=L)
    for a, b in zip(few, many):
        assert b.shape == (K, D * copies)
        assert torch.equal(a.repeat(1, copies), b)


def test_errors():
    from pb_bss_amd.evaluation import mir_eval_sources
    references, estimations = ob.gen_case(3, 2, 3, 300)
    with pytest.raises(NotImplementedError):
        mir_eval_sources(references, estimations, compute_permutation=False, filter_length=8)
    with pytest.raises(ValueError, match='Shapes do not fit'):
        mir_eval_sources(references[:1], estimations, filter_length=8)
    with pytest.raises(ValueError, match='Strange input shape'):
        mir_eval_sources(references[0], estimations[0], filter_length=8)
    silent = references.copy()
    silent[1] = 0
    with pytest.raises(ValueError, match='non-silent'):
        mir_eval_sources(silent, estimations, filter_length=8)
    silent = estimations.copy()
    silent[2] = 0
    with pytest.raises(ValueError, match='non-silent'):
        mir_eval_sources(references, silent, filter_length=8)
    with pytest.raises(NotImplementedError):
        mir_eval_sources(references, estimations, filter_length=513)


def test_output_metrics():
    from pb_bss_amd.evaluation import OutputMetrics
    references, estimations, expected, _ = generated(BIG_CASE)  # the classes use L = 512
    metrics = OutputMetrics(speech_prediction=estimations, speech_source=references,
                            enable_si_sdr=True)
    got = metrics.as_dict()
    assert list(got) == ['mir_eval_sdr', 'mir_eval_sir', 'mir_eval_sar', 'mir_eval_selection',
                         'si_sdr']
    diff = largest_difference([got['mir_eval_sdr'], got['mir_eval_sir'], got['mir_eval_sar']],
                              expected)
    print(f'OutputMetrics {BIG_CASE}: largest difference {diff:.3e} dB')
    assert diff < BOUND
    assert got['mir_eval_selection'].tolist() == expected[3].tolist()
    assert np.array_equal(metrics.speech_prediction_selection, estimations[expected[3]])
    assert got['si_sdr'].shape == (2,)


def test_input_metrics():
    from pb_bss_amd.evaluation import InputMetrics
    references, observation = input_metrics_case()
    K, D = len(references), len(observation)
    metrics = InputMetrics(observation=observation, speech_source=references)
    assert metrics.mir_eval_sdr.shape == (K, D)
    # channel d against source k: entry (d, k) of the table with the channels as estimates
    tables = ob.tables_direct(references, observation, BIG_CASE[3])
    expected = [table.T for table in tables]
    diff = largest_difference([metrics.mir_eval_sdr, metrics.mir_eval_sir, metrics.mir_eval_sar],
                              expected)
    print(f'InputMetrics (K=2, D=2, N=16000): largest difference {diff:.3e} dB')
    assert diff < BOUND
    assert list(metrics.as_dict()) == ['mir_eval_sdr', 'mir_eval_sir', 'mir_eval_sar']


def test_host_fallback_doctest_case():
    """periodic signals: cond(G) ~ 1.9e22 at K L = 1024"""
    from pb_bss_amd import _lib
    source, prediction = ob.doctest_signals()
    expected = ob.bss_eval(source, prediction, route='direct')
    got, _, status = evaluate(source, prediction, 512)
    assert status & _lib.ST_NOT_POSDEF
    diff = largest_difference(got, expected)
    recorded = max(np.abs(got[m] - ob.DOCTEST[name]).max()
                   for m, name in enumerate(('sdr', 'sir', 'sar')))
    print(f'doctest case: {diff:.3e} dB from the direct route, {recorded:.3e} dB from the '
          f'recorded values')
    assert got[3].tolist() == [0, 1]
    assert diff < FALLBACK_BOUND
    assert recorded < 1e-4


def test_host_fallback_dependent_references():
    """(3, 3, 1500, 24) with the third reference the sum of the first two"""
    from pb_bss_amd import _lib
    references, estimations = ob.gen_dependent_case(7)
    expected = ob.bss_eval(references, estimations, 24, route='direct')
    got, _, status = evaluate(references, estimations, 24)
    assert status & _lib.ST_NOT_POSDEF
    diff = largest_difference(got, expected)
    print(f'dependent references: largest difference {diff:.3e} dB')
    assert got[3].tolist() == expected[3].tolist()
    assert diff < FALLBACK_BOUND
