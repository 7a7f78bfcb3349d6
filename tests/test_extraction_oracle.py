"""CPU: the longdouble restatements of tests/oracle_extraction.py against oracle/beamformer.py and
oracle.cacgmm.normalize_observation in float64, at the cases and within the bounds of
tests/test_gpu_extraction_front_end.py, and the conditions those case lists have to meet: every
compiled instantiation has a case, the degenerate inputs are what their names say, the seams are
crossed, and no reference-channel case sits near a tie."""
import numpy as np
import pytest

import oracle_extraction as oe
from oracle import beamformer as ob
from oracle import cacgmm as oc

CUS = 256   # compute units assumed for the multi-trip batch here; the GPU test reads the device


def oracle_psd(x, mask, mode):
    m, normalize = oe.psd_mode_args(mask, mode)
    out = ob.psd(x.astype(np.complex128), m, normalize=normalize)
    return out[:, None] if m is None else out


def check_psd(x, mask, label, modes=oe.MODES):
    """Restatement against the float64 oracle in every mode; Hermitian to the bit on both sides
    is not asked of einsum, only the bound."""
    worst = 0.0
    T = x.shape[-1]
    for mode in modes:
        m, normalize = oe.psd_mode_args(mask, mode)
        ref = oe.psd(x, m, normalize)
        assert np.abs(ref - ref.conj().swapaxes(-1, -2)).max() == 0, (label, mode)
        ratio = oe.psd_ratio(oracle_psd(x, mask, mode), ref, T)
        assert ratio <= 1, (label, mode, ratio)
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize('D', oe.FUSED_D)
def test_psd_restatement_on_the_fused_grid(D):
    worst = 0.0
    for K in oe.FUSED_K:
        for dtype in oe.DTYPES:
            x, mask = oe.psd_input(D, K, oe.GRID_T, oe.GRID_B, dtype)
            assert x.dtype == dtype and x.shape == (oe.GRID_B, D, oe.GRID_T)
            flat = mask.reshape(-1, oe.GRID_T)
            assert len({r.tobytes() for r in flat}) == len(flat)   # every (b, k) its own mask
            worst = max(worst, check_psd(x, mask, (D, K, dtype)))
    print(f'D={D}: float64 oracle at {worst:.3f} of the bound')


def test_psd_restatement_on_the_frame_counts_and_edges():
    worst = 0.0
    for D, K in oe.FRAME_DK:
        for T in oe.FRAME_COUNTS:
            for dtype in oe.DTYPES:
                x, mask = oe.psd_input(D, K, T, oe.GRID_B, dtype)
                worst = max(worst, check_psd(x, mask, (D, K, T, dtype)))
    for D, K in oe.ROUTING_CASES:
        for dtype in oe.DTYPES:
            worst = max(worst, check_psd(*oe.routing_input(D, K, dtype), (D, K, dtype)))
    for dtype in oe.DTYPES:
        worst = max(worst, check_psd(*oe.degenerate_input(dtype), ('degenerate', dtype)))
    print(f'float64 oracle at {worst:.3f} of the bound')
    assert {T - 1 for T in oe.FRAME_COUNTS} >= {0, 63, 127, 191} and 1 in oe.FRAME_COUNTS
    assert all({m - 1, m, m + 1} <= set(oe.FRAME_COUNTS) for m in (64, 128, 192))
    assert oe.GRID_T > 64 and oe.GRID_T % 64 and oe.GRID_B > 1


@pytest.mark.parametrize('D', oe.GENERIC_D)
def test_psd_restatement_on_the_generic_grid(D):
    worst = 0.0
    for K in oe.GENERIC_K:
        T = oe.generic_frames(D, K)
        for dtype in oe.DTYPES:
            x, mask = oe.psd_input(D, K, T, oe.GENERIC_B, dtype)
            worst = max(worst, check_psd(x, mask, (D, K, T, dtype)))
    print(f'D={D}: float64 oracle at {worst:.3f} of the bound')


def test_psd_cases_reach_every_instantiation_and_route():
    # fused: psd_kernel<D, K, YS, SPILL> is compiled for D in 2..8, K in 1..4, both input types;
    # K = 5, 6 go out as 4 + 1 and 4 + 2 (launch_psd)
    assert set(oe.FUSED_D) == set(range(2, 9)) and set(oe.FUSED_K) == set(range(1, 7))
    assert set(oe.DTYPES) == {'complex64', 'complex128'} and len(oe.MODES) == 3
    assert {(D, K) for D, K in oe.ROUTING_CASES} == {(8, 6), (8, 7), (9, 1), (9, 6)}
    # generic: every T at every D and at every K; both class widths, all three sensor widths,
    # one launch, two, three and four launches, balanced
    for D in oe.GENERIC_D:
        assert {oe.generic_frames(D, K) for K in oe.GENERIC_K} == set(oe.GENERIC_T), D
    for K in oe.GENERIC_K:
        assert {oe.generic_frames(D, K) for D in oe.GENERIC_D} == set(oe.GENERIC_T), K
    widths = {16 if D <= 16 else 32 if D <= 32 else 36 for D in oe.GENERIC_D}
    assert widths == {16, 32, 36} and {16, 17, 32, 33, 34} <= set(oe.GENERIC_D)
    chunks = {K: oe.generic_chunks(K) for K in oe.GENERIC_K}
    assert chunks[7] == [4, 3] and chunks[13] == [5, 4, 4] and chunks[19] == [5, 5, 5, 4]
    assert all(sum(c) == K and max(c) <= 6 for K, c in chunks.items())
    assert {3 if kc <= 3 else 6 for c in chunks.values() for kc in c} == {3, 6}
    assert {len(c) for c in chunks.values()} == {1, 2, 3, 4}
    assert {63, 64, 65} <= set(oe.GENERIC_T) and max(oe.GENERIC_T) > 128
    assert {D for D, K in oe.REFUSED_DK} == {1, 8, 9, 35} and {K for D, K in oe.REFUSED_DK} == {1, 20}


def test_psd_bound_rejects_misplaced_and_slightly_wrong_results():
    """What the GPU sweep is there to catch, done to the float64 oracle's result by hand: classes
    or problems swapped, the transposed matrix, one entry off by 1e-12 of the diagonal, one frame
    left out, a residue of another mask, a nonzero where the output has to be exactly zero."""
    D, K, T, B = 5, 3, 70, 3
    x, mask = oe.psd_input(D, K, T, B, 'complex128')
    ref = oe.psd(x, mask, True)
    good = ob.psd(x, mask)
    assert oe.psd_ratio(good, ref, T) <= 1
    bad = {'classes swapped': good[:, [1, 0, 2]], 'problems swapped': good[[1, 0, 2]],
           'transposed': good.swapaxes(-1, -2).copy(),
           'a frame left out': ob.psd(x[..., :-1], mask[..., :-1]) * (mask[..., :-1].sum(-1)
                                                                    / mask.sum(-1))[..., None, None],
           'residue of another mask': good + 1e-11 * good[:, [1, 2, 0]]}
    off = good.copy()
    off[1, 2, 3, 1] += 1e-12 * off[1, 2].trace().real
    bad['one entry off'] = off
    for name, got in bad.items():
        assert oe.psd_ratio(got, ref, T) > 3, name
    zmask = mask.copy()
    zmask[0, 1] = 0
    zref = oe.psd(x, zmask, True)
    zgot = ob.psd(x, zmask)
    assert oe.psd_ratio(zgot, zref, T) <= 1
    zgot[0, 1, 2, 2] = 1e-300
    assert oe.psd_ratio(zgot, zref, T) == np.inf


def test_degenerate_masks_are_what_they_claim():
    (D, K), T = oe.DEGENERATE_DK, oe.DEGENERATE_T
    assert (D, K, T) == (6, 3, 130)
    for dtype in oe.DTYPES:
        x, mask = oe.degenerate_input(dtype)
        assert x.shape == (4, D, T) and mask.shape == (4, K, T) and (mask >= 0).all()
        assert (mask[0, 0] == 0).all()
        s = mask[0, 1].sum()
        assert 0 < s < oe.FLOOR and abs(s - 1e-13) < 1e-25 and (mask[0, 1] > 0).all()
        assert np.count_nonzero(mask[0, 2]) == 1
        assert mask[1].min() > 1e6 and mask[1].sum(-1).min() > 1e12
        zero = [t for t in range(T) if not x[2, :, t].any()]
        assert len(zero) == 20 and sorted(oe.ZERO_FRAMES) == zero
        assert all(x[b].all() for b in (0, 1, 3))
        ref = oe.psd(x, mask, True)
        assert (ref[0, 0] == 0).all() and oe.psd_bound(ref, T)[0, 0] == 0
        # the floor wins: sum (m / 1e-10) y y^H, a thousandth of a normalised class
        want = np.einsum('t,dt,et->de', mask[0, 1].astype(oe.LD) / oe.LD(oe.FLOOR),
                         oe.widen(x[0]), oe.widen(x[0]).conj())
        assert np.abs(ref[0, 1] - want).max() <= 2.0 ** -60 * np.abs(want).max()
        assert 0.5e-3 < ref[0, 1].trace().real / ref[3, 1].trace().real < 2e-3
        sv = np.linalg.svd(ref[0, 2].astype(np.complex128), compute_uv=False)
        assert sv[1] <= 1e-15 * sv[0]                               # rank one
        assert (oe.psd(np.zeros_like(x), mask, True) == 0).all()    # an all-zero input


def test_multi_trip_and_spill_cases():
    for D, K in oe.TRIP_DK:
        x, mask = oe.trip_input(D, K, 2)         # the pattern does not depend on the batch size
        B = oe.trip_batch(2)
        assert x.shape == (B, D, oe.TRIP_T) and x.dtype == np.complex64
        for b in range(B):
            zc = [k for k in range(K) if not mask[b, k].any()]
            zf = [t for t in range(oe.TRIP_T) if not x[b, :, t].any()]
            assert len(zc) == (b % 5 == 0) and len(zf) == (b % 7 == 0), b
        assert check_psd(x, mask, ('trips', D, K), modes=('normalized',)) <= 1
    # any grid of the launcher is at most MAX_WORKGROUPS_PER_CU * CUs workgroups
    assert oe.trip_batch(CUS) > 2 * oe.MAX_WORKGROUPS_PER_CU * CUS
    # the spilled variant: the frame arrays alone exceed the LDS of a compute unit
    want = {(8, 4, 'complex128'): 966, (8, 4, 'complex64'): 1542, (3, 2, 'complex128'): 1862}
    for D, K, dtype in oe.SPILL_CASES:
        T = oe.spill_frames(D, K, dtype)
        assert T == want[D, K, dtype] and T % 64 == 6
        assert oe.frame_bytes(D, K, dtype, T) > oe.LDS_LIMIT >= oe.frame_bytes(D, K, dtype, T - 64)
    assert oe.frame_bytes(8, 4, 'complex128', 966) == 4 * 1024 * 32 + 1024 * 8 + 4 * 1024 * 8
    assert oe.SPILL_TRIP_CASE in oe.SPILL_CASES
    assert set(oe.SPILL_CASES) == {(8, 4, 'complex128'), (8, 4, 'complex64'), (3, 2, 'complex128')}


def test_apply_restatement_and_seams():
    worst = 0.0
    cases = [(oe.APPLY_B, D, T, None) for D in oe.APPLY_D for T in oe.APPLY_T]
    cases += [oe.APPLY_STRIDE_CASE + (None,), oe.APPLY_SEAM_CASE + (None,),
              oe.APPLY_SHARED_SEAM_CASE + (oe.SHARED_X_BATCH,)]
    for B, D, T, x_batch in cases:
        for dtype in oe.DTYPES:
            w, x = oe.apply_input(B, D, T, dtype, x_batch)
            assert x.dtype == dtype and w.dtype == np.complex128
            x128 = x.astype(np.complex128)
            got = ob.apply_bf(w, x128 if x_batch is None else x128[np.arange(B) % x_batch])
            ratio = oe.apply_ratio(got, w, x)
            assert ratio <= 1, (B, D, T, dtype, ratio)
            worst = max(worst, ratio)
    print(f'float64 oracle at {worst:.3f} of the bound')
    assert max(oe.APPLY_D) == oe.APPLY_REFUSED_D - 1 and {1, 8, 9} <= set(oe.APPLY_D)
    assert {255, 256, 257} <= set(oe.APPLY_T)
    assert oe.APPLY_STRIDE_CASE[2] > 64 * 256            # a second trip of the frame loop
    assert oe.APPLY_SEAM_CASE[0] > oe.SEAM               # a second launch
    B, D, T = oe.APPLY_SHARED_SEAM_CASE
    assert B > oe.SEAM and B % oe.SHARED_X_BATCH == 0 and oe.SEAM % oe.SHARED_X_BATCH != 0
    # a wrong observation (any other residue) is far outside the bound for every problem
    w, x = oe.apply_input(B, D, T, 'complex128', oe.SHARED_X_BATCH)
    ref, bound = oe.apply_bf(w, x), oe.apply_bound(w, x)
    for shift in range(1, oe.SHARED_X_BATCH):
        other = oe.apply_bf(w, np.roll(x, -shift, axis=0))
        assert (np.abs(other - ref).max(axis=-1) > 1e6 * bound.max(axis=-1)).all(), shift


def test_normalize_restatement_and_edges():
    worst = 0.0
    cases = [(oe.NORMALIZE_B, T, D) for T in oe.NORMALIZE_T for D in oe.NORMALIZE_D]
    cases.append(oe.NORMALIZE_SEAM_CASE)
    for B, T, D in cases:
        for dtype in oe.DTYPES:
            y = oe.normalize_input(B, T, D, dtype)
            assert y.dtype == dtype
            y128 = y.astype(np.complex128)      # float64 on both sides
            got = oc.normalize_observation(y128)
            ratio = oe.normalize_ratio(got, y128)
            assert ratio <= 1, (B, T, D, dtype, ratio)
            worst = max(worst, ratio)
            zero = oe.normalize_zero_frames(T)
            assert (got[1][:, zero] == 0).all() and (oe.normalize(y)[1][:, zero] == 0).all()
            assert [t for t in range(T) if not y[1, t].any()] == zero
            assert all(y[b].any(axis=-1).all() for b in range(B) if b != 1)
    print(f'float64 oracle at {worst:.3f} of the bound')
    assert oe.normalize_zero_frames(130) == [0, 63, 64, 127, 128, 129]
    assert oe.normalize_zero_frames(64) == [0, 63] and oe.normalize_zero_frames(1) == [0]
    assert {63, 64, 65} <= set(oe.NORMALIZE_T) and {1, 8, 9, 34} <= set(oe.NORMALIZE_D)
    assert oe.NORMALIZE_SEAM_CASE[0] > oe.SEAM


def test_normalize_oracle_at_extreme_magnitudes():
    """What oracle.cacgmm.normalize_observation does where the squared norm leaves float64 (the
    device has to do the same): np.linalg.norm squares the entries, so a frame of magnitude
    1e-170 has norm 0, which eps_style='where' replaces by tiny -- the frame comes out as
    y / tiny, about 1e+137 -- and a frame of magnitude 1e+170 has norm Inf and comes out as 0."""
    y = oe.extreme_input()
    tiny_f, huge_f = list(oe.EXTREME_TINY), list(oe.EXTREME_HUGE)
    with np.errstate(over='ignore', under='ignore'):
        n2 = (y.real ** 2 + y.imag ** 2).sum(-1)
        assert (n2[:, tiny_f] == 0).all() and np.isinf(n2[:, huge_f]).all()
        got = oc.normalize_observation(y)
    assert y[:, tiny_f].all() and y[:, huge_f].all()
    tiny = np.finfo(np.float64).tiny
    assert (got[:, :, tiny_f] == (y[:, tiny_f] / tiny).swapaxes(-1, -2)).all()
    assert (y[:, tiny_f] * 2.0 ** 1022 == y[:, tiny_f] / tiny).all()    # 1 / tiny is exact
    assert 1e136 < np.abs(got[:, :, tiny_f]).max() < 1e139
    assert (got[:, :, huge_f] == 0).all()
    rest = [t for t in range(oe.EXTREME_T) if t not in tiny_f + huge_f]
    assert oe.normalize_ratio(got[:, :, rest], y[:, rest]) <= 1
    assert {63, 64} <= set(tiny_f)                                      # both sides of a tile edge


def oracle_snr(target, noise):
    """The SNR per candidate channel behind oracle.beamformer.mvdr_souden (one problem (F, D, D))."""
    eps = np.finfo(np.float64).tiny
    phi = ob.stable_solve(noise, target)
    lam = np.trace(phi, axis1=-1, axis2=-2)[..., None, None]
    mat = phi / np.maximum(lam.real, eps)
    num = np.einsum('FdR,FdD,FDR->R', mat.conj(), target, mat)
    den = np.einsum('FdR,FdD,FDR->R', mat.conj(), noise, mat)
    return num / np.maximum(den, eps)


def test_reference_channel_chain_cases_are_far_from_a_tie():
    assert (oe.CHAIN_L, oe.CHAIN_F, oe.CHAIN_D) == (3, 17, (3, 6, 8, 12))
    for D in oe.CHAIN_D:
        target, noise = oe.chain_input(D)
        assert target.shape == noise.shape == (oe.CHAIN_L, oe.CHAIN_F, D, D)
        for a in (target, noise):
            assert (a == a.conj().swapaxes(-1, -2)).all() and np.linalg.eigvalsh(a).min() > 0
        for l in range(oe.CHAIN_L):
            snr = oracle_snr(target[l], noise[l])
            assert np.isfinite(snr).all()
            _, ref = ob.mvdr_souden(target[l], noise[l], return_ref_channel=True)
            assert int(ref) == int(np.argmax(snr.real))
            top = np.sort(snr.real)[::-1]
            gap = (top[0] - top[1]) / abs(top[0])
            print(f'D={D} l={l}: reference channel {int(ref)}, gap {gap:.2e}')
            assert gap > oe.CHAIN_GAP, (D, l, gap)
