"""CPU: the NumPy restatement of WPE (tests/oracle_wpe.py) against two independent routes to the
same filter, its own error table against the copy the GPU test carries, the definitions of the
statistics modes and of psd_context by direct loops, the reach of the GPU sweep over the kernels'
plan (engine.WPE_*), and the public surface (names, header, bindings)."""
import importlib
import os
import re

import numpy as np
import pytest

import oracle_wpe as ow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def measured():
    """{case: (e_case after one iteration, after three)}: the largest over both statistics modes
    and both input dtypes, for exactly the inputs of the GPU sweep."""
    table = {}
    for case in ow.CASES:
        e = [ow.measure_e_case(case, dtype, mode)
             for dtype in (np.complex128, np.complex64) for mode in ('full', 'valid')]
        table[case] = (max(x[0] for x in e), max(x[1] for x in e))
    return table


def test_restatement_against_weighted_least_squares(measured):
    """One iteration: normal equations + pivoted LU against lstsq on the scaled stacked frames.
    Both are backward stable routes to the same filter; the normal equations carry the larger
    error, cond(R) eps, which is what e_case measures, so the distance obeys the device bound."""
    for case in ow.CASES:
        D, taps, delay, T = case
        Y = ow.case_input(case)
        for mode in ('full', 'valid'):
            a = ow.wpe(Y, taps, delay, 1, 0, mode)
            b = ow.wpe_lstsq(Y, taps, delay, 1, 0, mode)
            dist = np.abs(a - b).max() / np.abs(a).max()
            print(f'{case} {mode}: lstsq distance {dist:.1e}, e_case {measured[case][0]:.1e}')
            assert dist <= 16 * max(measured[case][0], 1e-13), (case, mode, dist)


def test_e_case_table_matches_the_gpu_files_copy(measured):
    import test_gpu_wpe as gpu
    assert set(gpu.E_CASE) == set(ow.CASES)
    print('(D, taps, delay, T): measured e_case 1 / 3 iterations | table')
    for case in ow.CASES:
        m, tab = measured[case], gpu.E_CASE[case]
        print(f'{case}: {m[0]:.1e} {m[1]:.1e} | {tab[0]:.1e} {tab[1]:.1e}')
    for case in ow.CASES:
        for m, tab in zip(measured[case], gpu.E_CASE[case]):
            assert tab <= 4 * m, (case, m, tab)   # the table may not exceed the measurement ...
            assert m <= 4 * tab, (case, m, tab)   # ... nor fall far below it
    # the domain of the sweep: T >= 3 M wherever M >= 60
    for D, taps, delay, T in ow.CASES:
        assert D * taps < 60 or T >= 3 * D * taps


def test_statistics_modes_differ_by_the_dropped_frames():
    D, taps, delay, T = 3, 4, 2, 40
    Y = ow.synth(1, D, T, seed=5)[0]
    inv = ow.power_inverse(Y)
    Rf, Pf = ow.correlations(Y, inv, taps, delay, 'full')
    Rv, Pv = ow.correlations(Y, inv, taps, delay, 'valid')
    Rd = np.zeros_like(Rf)
    Pd = np.zeros_like(Pf)
    for t in range(delay + taps - 1):      # the frames 'valid' drops, summed by hand
        yt = np.zeros(D * taps, np.complex128)
        for k in range(taps):
            if t - delay - k >= 0:
                yt[k * D:(k + 1) * D] = Y[:, t - delay - k]
        Rd += inv[t] * np.outer(yt, yt.conj())
        Pd += inv[t] * np.outer(yt, Y[:, t].conj())
    assert np.abs(Rd).max() > 0 and np.abs(Pd).max() > 0
    assert np.abs(Rf - Rv - Rd).max() <= 8 * T * 2.0 ** -52 * np.abs(Rf).max()
    assert np.abs(Pf - Pv - Pd).max() <= 8 * T * 2.0 ** -52 * np.abs(Pf).max()
    assert np.abs(Rf - Rf.conj().T).max() <= 8 * T * 2.0 ** -52 * np.abs(Rf).max()


@pytest.mark.parametrize('context', [0, 2, np.inf])
def test_psd_context_against_a_direct_loop(context):
    D, T = 3, 17
    X = ow.synth(2, D, T, seed=9)
    X[1, :, 5:9] *= 1e-7                   # a stretch that reaches the 1e-10 floor
    p = (np.abs(X) ** 2).sum(axis=1) / D
    want = np.empty((2, T))
    for b in range(2):
        for t in range(T):
            frames = [u for u in range(T) if context == np.inf or abs(u - t) <= context]
            want[b, t] = sum(p[b, u] for u in frames) / len(frames)
    np.testing.assert_allclose(ow.power(X, context), want, rtol=1e-14)
    inv = ow.power_inverse(X, context)
    want_inv = 1 / np.maximum(want, 1e-10 * want.max(axis=-1, keepdims=True))
    np.testing.assert_allclose(inv, want_inv, rtol=1e-14)
    if context == 0:
        assert (inv[1, 5:9] == 1 / (1e-10 * ow.power(X)[1].max())).all()
        assert (inv[1, 5:9] == inv[1].max()).all() and (inv[1, :5] < inv[1].max()).all()
    assert (ow.power_inverse(np.zeros((D, T), np.complex128), context) == 0).all()


def test_gpu_sweep_reaches_every_boundary_of_the_plan():
    from pb_bss_amd import engine
    Ds = {c[0] for c in ow.CASES}
    Ms = {c[0] * c[1] for c in ow.CASES}
    Ts = {c[3] for c in ow.CASES}
    assert 1 in Ds and engine.WPE_MAX_D in Ds and engine.WPE_MAX_M in Ms
    for bound in engine.WPE_APPLY_D:       # the filter instantiations: at and just above each
        assert bound in Ds and (bound == engine.WPE_MAX_D or bound + 1 in Ds), bound
    for length in (engine.WPE_SPAN, engine.WPE_APPLY_FRAMES):
        assert {length - 1, length, length + 1} <= Ts, length
    assert any(T > 2 * engine.WPE_SPAN for T in Ts)   # more than two spans to add up
    per_wave = {engine.wpe_corr_tiles_per_wave(c[0], c[1]) for c in ow.CASES}
    blocks = range(1, -(-(engine.WPE_MAX_M + engine.WPE_MAX_D) // engine.WPE_TILE) + 1)
    possible = sorted({-(-(n * (n + 1) // 2) // 4) for n in blocks})
    for bound in engine.WPE_CORR_TILES:    # every correlation instantiation: at its bound and at
        above = [n for n in possible if n > bound]   # the next tile count there is
        assert bound in per_wave and (not above or above[0] in per_wave), bound
    assert engine.wpe_corr_tiles_per_wave(engine.WPE_MAX_D, engine.WPE_MAX_M // engine.WPE_MAX_D) \
        <= engine.WPE_CORR_TILES[-1]
    assert engine.wpe_corr_tiles_per_wave(1, engine.WPE_MAX_M) <= engine.WPE_CORR_TILES[-1]
    # an extended Gram matrix that is no multiple of the tile, and one that is
    edges = {(c[0] * c[1] + c[0]) % engine.WPE_TILE for c in ow.CASES}
    assert 0 in edges and len(edges) > 3
    assert ow.BATCH > 1
    for D, taps in ((8, 12), (16, 6), (1, 96)):
        assert engine.wpe_solve_lds(D, taps) <= engine.WPE_LDS


def test_public_surface():
    from pb_bss_amd import _lib, transform
    module = importlib.import_module('pb_bss_amd.transform.wpe')
    names = ['wpe', 'get_power', 'get_power_inverse', 'get_correlations', 'get_filter_matrix',
             'perform_filter_operation']
    for name in names:
        assert getattr(transform, name) is getattr(module, name) and name in transform.__all__
    with open(os.path.join(ROOT, 'include', 'pbbss.h')) as f:
        header = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    for export in ('pbbss_wpe', 'pbbss_wpe_correlations', 'pbbss_wpe_apply_filter',
                   'pbbss_wpe_power_inverse', 'pbbss_wpe_filter_matrix'):
        assert re.search(r'\b' + export + r'\s*\(', header), export
        assert export in _lib.SIGNATURES, export
    assert 'nara_wpe' in module.__doc__ and 'NOT checked' in ow.__doc__
