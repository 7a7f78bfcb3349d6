"""GPU: the extraction front end -- pbbss_psd (fused psd_kernel and generic gen_cov_kernel),
pbbss_apply_beamforming_vector[_shared], pbbss_normalize_observation and the
mvdr_souden -> select_reference_channel chain -- through pb_bss_amd.engine against the longdouble
restatements of tests/oracle_extraction.py, within the bounds derived there (eps = 2^-52):

    PSD        |got - ref|_max <= (2 T + 16) eps max_i Re ref[b, k, i, i], exact zeros where the
               bound is 0, and out == out^H to the bit
    apply      |got - ref| <= (D + 3) eps sum_d |w_d| |x_dt|
    normalize  |got - ref| <= (D + 4) eps per component (complex64: against the reference rounded
               to float32, plus 2^-23 |ref|); all-zero frames stay exactly zero
    reference channel: index and flag exact, the gathered column bit-equal to the matrix column

A correct kernel cannot exceed them; every test prints the worst err / bound it saw.

Where the cases come from (csrc/beamform.hip, csrc/capi_bf.hip, csrc/generic.hip):
  * psd_kernel<D, K, YS, SPILL> is compiled for D in 2..8, K in 1..4 and both input types;
    launch_psd sends K = 5, 6 as 4 + (K - 4).  The grid test runs every (D, K, type) in all three
    modes with a mask of its own per (b, k).
  * The persistent loop `for (b = blockIdx.x; b < B; b += gridDim.x)`: a CDNA4 compute unit holds
    at most 32 wavefronts (maxThreadsPerMultiProcessor = 2048), that is 8 four-wave workgroups,
    so the launcher's grid CUs * occupancy is at most 8 CUs and B = 16 CUs + 3 problems send
    every workgroup round the loop at least twice, whatever occupancy the runtime reports.
  * SPILL: EmKernel::frame_bytes(T) = DP Tp 4 sizeof(YS) + Tp 8 + K Tp 8 with DP = (D + 1) / 2,
    Tp = T rounded up to 64, against the handle's LDS limit, 160 KiB = 163 840 B on gfx950:
      (8, 4, complex128): 4 * 4 * 8 + 8 + 32 = 168 B a frame; 960 * 168 = 161 280 fits,
                          1024 * 168 = 172 032 does not: T = 960 + 6 = 966 (Tp = 1024)
      (8, 4, complex64):  104 B a frame; 1536 * 104 = 159 744, 1600 * 104 = 166 400: T = 1542
      (3, 2, complex128): 88 B a frame; 1856 * 88 = 163 328, 1920 * 88 = 168 960: T = 1862
    The frame arrays alone exceed the limit there, so lds_bytes(T) does whatever the small
    matrices take.  (3, 2, complex128) runs again at 16 CUs + 3 problems: 4099 * 3 * 1862
    complex128 are 366 MB, and the longdouble reference of it takes about two seconds.
  * gen_cov_kernel<DP, KM, YS>: DP in {16, 32, 36}, KM in {3, 6}, 64-frame tiles, balanced chunks
    of at most 6 classes; pbbss_psd routes D > 8 or K > 6 there.
  * apply_kernel strides over T beyond 64 * 256 frames; capi_bf.hip and capi_comm.hip cut the
    batch at the 65 535 limit of grid.y, and the shared call passes b_first so that problem b
    reads x[(b_first + b) % x_batch].
  * normalize_kernel: 64-frame LDS tile with leading dimension D + 1.  Where the squared norm
    leaves float64 the kernel does what oracle.cacgmm.normalize_observation (np.linalg.norm, then
    eps_style='where') does: a frame of magnitude 1e-170 has norm 0 there and comes out as
    y / tiny (about 1e+137), a frame of magnitude 1e+170 has norm Inf and comes out as 0.

Worst err / bound on an MI355X (gfx950, 256 compute units: B = 4099 in the multi-trip tests), the
run this change was made with:
    psd fused grid, D = 2..8          0.010 0.010 0.011 0.010 0.011 0.010 0.011
    psd frame counts                  (3, 2): 0.057   (8, 4): 0.076
    psd trips, B = 4099               (3, 2): 0.014   (8, 4): 0.015
    psd spilled, B = 3                (8, 4, complex128) T = 966: 0.001
                                      (8, 4, complex64) T = 1542: < 0.0005
                                      (3, 2, complex128) T = 1862: < 0.0005
    psd spilled trips, B = 4099       (3, 2, complex128) T = 1862: 0.001
    psd degenerate masks              0.005
    psd routing boundary              0.025
    psd generic grid, D = 9..34       0.025 0.024 0.023 0.023 0.026 0.024
    apply                             grid 0.218, T = 16 684: 0.204, batch seam 0.231,
                                      shared batch seam 0.240
    normalize                         grid 0.194, batch seam 0.208, beside extreme frames 0.096
    reference channel chain           vector error 3.6e-16 .. 1.6e-15 of the 1e-10 allowed
"""
import ctypes

import numpy as np
import pytest

import oracle_extraction as oe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def engine():
    from pb_bss_amd import _lib, engine
    _lib.require_gpu()
    return engine


def dev(x):
    from pb_bss_amd import _lib
    return _lib.to_device(x)


def host(x):
    from pb_bss_amd import _lib
    return _lib.to_host(x)


def device_properties():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device())


def compute_units():
    props = device_properties()
    # the premise of the multi-trip batch: at most 8 four-wave workgroups on a compute unit
    assert getattr(props, 'max_threads_per_multi_processor', 2048) // 256 \
        <= oe.MAX_WORKGROUPS_PER_CU
    return props.multi_processor_count


def lds_limit():
    """What csrc/handle.hip takes as the limit: the LDS of a compute unit."""
    props = device_properties()
    return max(getattr(props, 'shared_memory_per_multiprocessor', 0), props.shared_memory_per_block,
               oe.LDS_LIMIT)


def raw():
    """(library, handle, pointer-of) for calls past the Python layer."""
    from pb_bss_amd import _lib
    return _lib.load(), _lib.handle(0), lambda a: ctypes.c_void_p(a.data_ptr())


# ---- PSD ----------------------------------------------------------------------------------------
def device_psd(engine, x, mask, mode):
    m, normalize = oe.psd_mode_args(mask, mode)
    out = host(engine.psd(dev(x), None if m is None else dev(m), normalize=normalize))
    K = 1 if m is None else m.shape[1]
    assert out.dtype == np.complex128 and out.shape == (x.shape[0], K) + (x.shape[1],) * 2
    assert (out == out.conj().swapaxes(-1, -2)).all(), 'Hermitian to the bit'
    return out


def check_psd(engine, x, mask, label, modes=oe.MODES):
    """Worst err / bound over `modes`; asserts the bound, the exact zeros and the symmetry."""
    worst = 0.0
    for mode in modes:
        ref = oe.psd(x, *oe.psd_mode_args(mask, mode))
        ratio = oe.psd_ratio(device_psd(engine, x, mask, mode), ref, x.shape[-1])
        assert ratio <= 1, (label, mode, ratio)
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize('D', oe.FUSED_D)
def test_psd_fused_grid(engine, D):
    """Every compiled (D, K, input type) of the fused kernel, K = 5 and 6 as two launches, in all
    three modes; B = 3, T = 70: two chunks, the last one partial."""
    worst = 0.0
    for K in oe.FUSED_K:
        for dtype in oe.DTYPES:
            x, mask = oe.psd_input(D, K, oe.GRID_T, oe.GRID_B, dtype)
            worst = max(worst, check_psd(engine, x, mask, (D, K, dtype)))
    print(f'RATIO psd fused grid D={D}: {worst:.3f}')


@pytest.mark.parametrize('D,K', oe.FRAME_DK)
def test_psd_frame_counts(engine, D, K):
    worst = 0.0
    for T in oe.FRAME_COUNTS:
        for dtype in oe.DTYPES:
            x, mask = oe.psd_input(D, K, T, oe.GRID_B, dtype)
            worst = max(worst, check_psd(engine, x, mask, (D, K, T, dtype)))
    print(f'RATIO psd frame counts ({D}, {K}): {worst:.3f}')


@pytest.mark.parametrize('D,K', oe.TRIP_DK)
def test_psd_second_and_third_trip_of_the_persistent_loop(engine, D, K):
    """B = 16 CUs + 3 problems, each with its own data; an all-zero class where b % 5 == 0 and an
    all-zero frame where b % 7 == 0: what a workgroup leaves in LDS (cpack, red, flags, the zero
    padding of wbuf) differs from what its next problem needs."""
    x, mask = oe.trip_input(D, K, compute_units())
    assert x.shape[0] == 16 * compute_units() + 3
    worst = check_psd(engine, x, mask, ('trips', D, K), modes=('normalized',))
    print(f'RATIO psd trips ({D}, {K}) B={x.shape[0]}: {worst:.3f}')


@pytest.mark.parametrize('D,K,dtype', oe.SPILL_CASES)
def test_psd_spilled_variant(engine, D, K, dtype):
    """The frame arrays in the per-workgroup scratch slab: the smallest 64 m + 6 frames that no
    longer fit the LDS (module docstring), B = 3."""
    T = oe.spill_frames(D, K, dtype, lds_limit())
    assert oe.frame_bytes(D, K, dtype, T) > lds_limit()
    x, mask = oe.psd_input(D, K, T, oe.GRID_B, dtype)
    worst = check_psd(engine, x, mask, ('spill', D, K, dtype, T))
    print(f'RATIO psd spilled ({D}, {K}, {dtype}) T={T}: {worst:.3f}')


def test_psd_spilled_variant_over_several_trips(engine):
    """One spilled case at the batch of the multi-trip test: every workgroup reuses its scratch
    slab.  The reference stays longdouble (about two seconds)."""
    D, K, dtype = oe.SPILL_TRIP_CASE
    T = oe.spill_frames(D, K, dtype, lds_limit())
    x, mask = oe.trip_input(D, K, compute_units(), T=T, dtype=dtype)
    worst = check_psd(engine, x, mask, ('spill trips', D, K, dtype, T), modes=('normalized',))
    print(f'RATIO psd spilled trips ({D}, {K}, {dtype}) T={T} B={x.shape[0]}: {worst:.3f}')


def test_psd_degenerate_masks(engine):
    (D, K), T = oe.DEGENERATE_DK, oe.DEGENERATE_T
    worst = 0.0
    for dtype in oe.DTYPES:
        x, mask = oe.degenerate_input(dtype)
        worst = max(worst, check_psd(engine, x, mask, ('degenerate', dtype)))
        got = device_psd(engine, x, mask, 'normalized')
        assert (got[0, 0] == 0).all()                      # the all-zero class: exactly zero
        ref = oe.psd(x, mask, True)
        sv = np.linalg.svd(got[0, 2], compute_uv=False)    # one frame: rank one
        assert sv[1] <= D * oe.psd_bound(ref, T)[0, 2]
        # the class below the floor is divided by 1e-10, not by its sum
        scale = got[0, 1].trace().real / device_psd(engine, x, mask, 'plain')[0, 1].trace().real
        assert abs(scale * oe.FLOOR - 1) < 1e-12
        zero = host(engine.psd(dev(np.zeros_like(x)), dev(mask)))
        assert (zero == 0).all()                           # an all-zero input
    print(f'RATIO psd degenerate masks: {worst:.3f}')


def test_psd_routing_boundary(engine):
    """(8, 6) is the last fused shape, (8, 7), (9, 1) and (9, 6) the first generic ones: the same
    restatement on both sides, and the six classes the K = 6 and K = 7 calls at D = 8 share
    agree within the sum of both bounds."""
    worst = 0.0
    for dtype in oe.DTYPES:
        for D, K in oe.ROUTING_CASES:
            x, mask = oe.routing_input(D, K, dtype)
            worst = max(worst, check_psd(engine, x, mask, (D, K, dtype)))
        for mode in ('normalized', 'plain'):
            x, m7 = oe.routing_input(8, 7, dtype)
            _, m6 = oe.routing_input(8, 6, dtype)
            assert (m7[:, :6] == m6).all()
            fused, generic = device_psd(engine, x, m6, mode), device_psd(engine, x, m7, mode)
            bound = oe.psd_bound(oe.psd(x, *oe.psd_mode_args(m6, mode)), oe.ROUTING_T)
            err = np.abs(generic[:, :6] - fused).max(axis=(-1, -2))
            assert (err <= 2 * bound).all(), (dtype, mode, (err / bound).max())
            worst = max(worst, float((err / (2 * bound)).max()))
    print(f'RATIO psd routing boundary: {worst:.3f}')


@pytest.mark.parametrize('D', oe.GENERIC_D)
def test_psd_generic_grid(engine, D):
    """gen_cov_kernel: all three sensor widths, both class widths, one to four launches per call,
    T around its 64-frame tile; B = 2, both input types, all three modes."""
    worst = 0.0
    for K in oe.GENERIC_K:
        T = oe.generic_frames(D, K)
        for dtype in oe.DTYPES:
            x, mask = oe.psd_input(D, K, T, oe.GENERIC_B, dtype)
            worst = max(worst, check_psd(engine, x, mask, (D, K, T, dtype)))
    print(f'RATIO psd generic grid D={D}: {worst:.3f}')


def test_psd_refuses_what_no_kernel_serves(engine):
    """D = 1, D = 35 and K = 20: NotImplementedError from the engine (PBBSS_ERR_UNSUPPORTED at the
    ABI), and nothing written to the output."""
    from pb_bss_amd import _lib
    t = _lib.torch()
    lib, h, p = raw()
    B, T = 2, 70
    for D, K in oe.REFUSED_DK:
        x, mask = oe.psd_input(D, K, T, B, 'complex128')
        xd, md = dev(x), dev(mask)
        with pytest.raises(NotImplementedError):
            engine.psd(xd, md)
        out = t.full((B, K, D, D), 7.0, dtype=t.complex128, device='cuda')
        assert lib.pbbss_psd(h, p(xd), 1, B, T, D, K, p(md), 1, p(out), None) == _lib.ERR_UNSUPPORTED
        t.cuda.synchronize()
        assert bool((out == 7.0).all()), (D, K)


# ---- apply --------------------------------------------------------------------------------------
def check_apply(engine, B, D, T, dtype, x_batch=None):
    w, x = oe.apply_input(B, D, T, dtype, x_batch)
    got = host(engine.apply_bf(dev(w), dev(x)))
    assert got.dtype == np.complex128 and got.shape == (B, T)
    ratio = oe.apply_ratio(got, w, x)
    assert ratio <= 1, (B, D, T, dtype, x_batch, ratio)
    return ratio


def test_apply_grid(engine):
    worst = 0.0
    for D in oe.APPLY_D:
        for T in oe.APPLY_T:
            for dtype in oe.DTYPES:
                worst = max(worst, check_apply(engine, oe.APPLY_B, D, T, dtype))
    print(f'RATIO apply grid: {worst:.3f}')


def test_apply_second_trip_of_the_frame_loop(engine):
    worst = max(check_apply(engine, *oe.APPLY_STRIDE_CASE, dtype) for dtype in oe.DTYPES)
    print(f'RATIO apply T={oe.APPLY_STRIDE_CASE[2]}: {worst:.3f}')


def test_apply_across_the_batch_seam(engine):
    """B = 65 537: the second launch starts at problem 65 535 of w, x and out."""
    worst = max(check_apply(engine, *oe.APPLY_SEAM_CASE, dtype) for dtype in oe.DTYPES)
    print(f'RATIO apply batch seam: {worst:.3f}')


def test_apply_shared_across_the_batch_seam(engine):
    """65 541 vectors on 7 clearly different observations: 65 535 % 7 = 1, so the second launch
    starts in the middle of an observation and only b_first keeps problem b on x[b % 7]."""
    worst = max(check_apply(engine, *oe.APPLY_SHARED_SEAM_CASE, dtype, oe.SHARED_X_BATCH)
                for dtype in oe.DTYPES)
    print(f'RATIO apply shared batch seam: {worst:.3f}')


def test_apply_refuses_thirty_sensors(engine):
    """beamformer.py:582: PBBSS_ERR_INVALID_ARG at the ABI with the output untouched, the
    reference's AssertionError from the wrapper."""
    from pb_bss_amd import _lib, extraction
    t = _lib.torch()
    lib, h, p = raw()
    B, D, T = 3, oe.APPLY_REFUSED_D, 5
    w, x = oe.apply_input(B, D, T, 'complex128')
    wd, xd = dev(w), dev(x)
    out = t.full((B, T), 7.0, dtype=t.complex128, device='cuda')
    rc = lib.pbbss_apply_beamforming_vector(h, p(wd), p(xd), 1, B, T, D, p(out), None)
    assert rc == _lib.ERR_INVALID_ARG
    rc = lib.pbbss_apply_beamforming_vector_shared(h, p(wd), p(xd), 1, B, 1, T, D, p(out), None)
    assert rc == _lib.ERR_INVALID_ARG
    t.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(AssertionError):
        extraction.apply_beamforming_vector(w, x)


# ---- normalize ----------------------------------------------------------------------------------
def check_normalize(engine, B, T, D, dtype):
    y = oe.normalize_input(B, T, D, dtype)
    got = host(engine.normalize_observation(dev(y)))
    ratio = oe.normalize_ratio(got, y)
    assert ratio <= 1, (B, T, D, dtype, ratio)
    assert (got[1][:, oe.normalize_zero_frames(T)] == 0).all()   # zero frames stay exactly zero
    return ratio


def test_normalize_grid(engine):
    worst = 0.0
    for T in oe.NORMALIZE_T:
        for D in oe.NORMALIZE_D:
            for dtype in oe.DTYPES:
                worst = max(worst, check_normalize(engine, oe.NORMALIZE_B, T, D, dtype))
    print(f'RATIO normalize grid: {worst:.3f}')


def test_normalize_across_the_batch_seam(engine):
    worst = max(check_normalize(engine, *oe.NORMALIZE_SEAM_CASE, dtype) for dtype in oe.DTYPES)
    print(f'RATIO normalize batch seam: {worst:.3f}')


def test_normalize_where_the_squared_norm_leaves_float64(engine):
    """Frames of magnitude 1e-170 and 1e+170 (complex128): the device does what
    oracle.cacgmm.normalize_observation does, to the bit -- y / tiny where the squared norm
    underflows to 0, 0 where it overflows -- and the other frames keep the bound."""
    from oracle import cacgmm as oc
    y = oe.extreme_input()
    with np.errstate(over='ignore', under='ignore'):
        want = oc.normalize_observation(y)
    got = host(engine.normalize_observation(dev(y)))
    tiny_f, huge_f = list(oe.EXTREME_TINY), list(oe.EXTREME_HUGE)
    assert (got[:, :, tiny_f] == want[:, :, tiny_f]).all() and np.abs(want[:, :, tiny_f]).min() > 1e130
    assert (got[:, :, huge_f] == 0).all() and (want[:, :, huge_f] == 0).all()
    rest = [t for t in range(oe.EXTREME_T) if t not in tiny_f + huge_f]
    ratio = oe.normalize_ratio(got[:, :, rest], y[:, rest])
    assert ratio <= 1, ratio
    print(f'RATIO normalize extreme magnitudes, ordinary frames: {ratio:.3f}')


# ---- reference channel --------------------------------------------------------------------------
@pytest.mark.parametrize('D', oe.CHAIN_D)
def test_reference_channel_chain_against_the_oracle(engine, D):
    """Hermitian positive-definite (target, noise) -> engine.mvdr_souden ->
    engine.select_reference_channel against oracle.beamformer.mvdr_souden per problem: the index
    exact (tests/test_extraction_oracle.py keeps every case a relative 1e-6 away from a tie), the
    vector within the 1e-10 of test_mvdr_ban_apply, the column gather to the bit."""
    from oracle import beamformer as ob
    target, noise = oe.chain_input(D)
    L, F = oe.CHAIN_L, oe.CHAIN_F
    eps = float(np.finfo(np.float64).tiny)
    mat, num, den, st = engine.mvdr_souden(dev(np.array(target.reshape(L * F, D, D))),
                                           dev(np.array(noise.reshape(L * F, D, D))), eps)
    assert (host(st) == 0).all()
    w, ref, ok = engine.select_reference_channel(mat, num, den, L, F, eps)
    w, mat = host(w), host(mat).reshape(L, F, D, D)
    assert ok.tolist() == [1] * L
    worst = 0.0
    for l in range(L):
        want_w, want_ref = ob.mvdr_souden(target[l], noise[l], return_ref_channel=True)
        assert int(ref[l]) == int(want_ref), (D, l)
        np.testing.assert_array_equal(w[l], mat[l, :, :, int(want_ref)])
        err = np.abs(w[l] - want_w).max() / np.abs(want_w).max()
        assert err < 1e-10, (D, l, err)
        worst = max(worst, err)
    print(f'RATIO reference channel chain D={D}: vector error {worst:.2e} (tolerance 1e-10)')
