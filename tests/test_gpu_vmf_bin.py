"""GPU: the per-bin von-Mises-Fisher mixture kernel (csrc/vmf_bin.hip) and the vMF normaliser over
their domain, against the float64 oracle (oracle/embed.py) on the inputs of
tests/oracle_vmf_bin.py.

What the kernel writes by hand -- the tabulated log-Bessel polynomial and its block size, series
logarithm and exponential, Newton reciprocals, the feature count padded to a template parameter,
the split over four or eight wavefronts -- is reached here at every block size, at both clamps of
the concentration, in every compiled shape and on both sides of every route boundary.  The
normaliser is no output: probe rows with saliency 0 whose oracle posterior lies in (0.05, 0.95)
make an error delta of an offset visible as up to delta / 4 of a posterior (oracle_vmf_bin.py).

Tolerances are the project's (tests/test_gpu_embed.py): mean 1e-9, concentration
1e-8 relative, weight 1e-10, posteriors 1e-9 after one step and 1e-8 after a trajectory, the
log-normaliser rtol 1e-12 / atol 2e-12.  tests/test_vmf_bin_oracle.py bounds the oracle's own
error (1e-13 relative in the log-normaliser) and checks what every scenario promises.
"""
import functools

import numpy as np
import pytest

import oracle_vmf_bin as vb
from oracle import embed as oe

pytestmark = pytest.mark.gpu

ALL = [(name, param) for name, lst in vb.CASES.items() for param, _ in lst]
DTYPES = ('float32', 'float64')
STEP = dict(mean=1e-9, conc=1e-8, weight=1e-10, aff=1e-9)        # one EM step
TRAJECTORY = dict(mean=1e-9, conc=1e-8, weight=1e-10, aff=1e-8)  # several


def device_fit(y, init, sal, iterations, cmin=1e-10, cmax=500.0, weight_mode=0):
    """engine.vmfmm_fit with the final E-step -> host arrays (weight as (B, K, 1))."""
    from pb_bss_amd import _lib, engine
    dev = lambda a: None if a is None else _lib.to_device(np.array(a))  # noqa: E731
    r = engine.vmfmm_fit(dev(y), init.shape[1], gamma0=dev(init), iterations=iterations,
                         saliency=dev(sal), weight_mode=weight_mode, min_concentration=cmin,
                         max_concentration=cmax, final_predict=True)
    out = {k: _lib.to_host(r[k]) for k in ('mean', 'concentration', 'weight', 'affiliation')}
    out['weight'] = out['weight'][..., None]
    return out


def assert_close(got, ref, tol, what='', affiliation=None, weight=True):
    """Model (and posteriors) within `tol`; NaN exactly where the reference has them."""
    np.testing.assert_allclose(got['mean'], ref['mean'], rtol=0, atol=tol['mean'], err_msg=what)
    np.testing.assert_allclose(got['concentration'], ref['concentration'], rtol=tol['conc'],
                               atol=0, err_msg=what)
    if weight:
        np.testing.assert_allclose(got['weight'], ref['weight'], rtol=0, atol=tol['weight'],
                                   err_msg=what)
    if affiliation is not None:
        np.testing.assert_allclose(got['affiliation'], affiliation, rtol=0, atol=tol['aff'],
                                   err_msg=what)


def assert_clamped(got, c):
    """A concentration the scenario promises beyond a clamp IS the clamp, bit for bit."""
    for k, promise in enumerate(c['promise']):
        if promise == 'high':
            assert (got['concentration'][:, k] == c['cmax']).all(), got['concentration'][:, k]
        elif promise == 'low':
            assert (got['concentration'][:, k] == c['cmin']).all(), got['concentration'][:, k]
        else:
            assert (got['concentration'][:, k] > c['cmin']).all()
            assert (got['concentration'][:, k] < c['cmax']).all()


def logit_error(got, c):
    """max |logit(gamma_dev) - logit(gamma_oracle)| of class 0 over the probe rows: the error of
    offset_0 - offset_1 (plus that of the dot products) as the posterior shows it."""
    P = c['P']
    with np.errstate(all='ignore'):
        return float(np.abs(vb.logit(got['affiliation'][:, 0, -P:]) -
                            vb.logit(c['affiliation'][:, 0, -P:])).max())


# ---- a. the normaliser through probes ----------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('E', vb.E_LIST)
@pytest.mark.parametrize('name,param', ALL)
def test_normaliser_through_probes(name, param, E, dtype):
    """One EM step and the final E-step of the per-bin kernel (B = 16) at every block size of the
    tabulated polynomial (bR = 1, 2, 9, 10, 16), past its hand-over to the generic series, with a
    class on the upper clamp, on the lower clamp and between them: model at the single-step
    tolerances, a clamped concentration EQUAL to the clamp, posteriors of the probe rows (oracle
    posterior in (0.05, 0.95)) to 1e-9.  The logit error is printed; 1e-9 / 0.0475 = 2.1e-8 is the
    most atol 1e-9 lets through.  Measured: 1e-14 (cap 10) ... 1e-12 (cap 960) and 2e-12 (cap 2000)
    with class 0 on the cap -- eps times the concentration -- and up to 1.3e-10 with a free
    concentration of 900, where the error of the concentration itself shows (the sweep route:
    1.4e-11)."""
    c = vb.case(name, param, E, dtype)
    got = device_fit(c['y'], c['init'], c['saliency'], 1, c['cmin'], c['cmax'])
    err = logit_error(got, c)
    print(f'LOGIT {name} {param} E={E} {dtype}: {err:.2e}')
    what = f'{name} {param} E={E} {dtype}'
    assert_close(got, c['model'], STEP, what, affiliation=c['affiliation'])
    assert_clamped(got, c)


# ---- b. two device routes on the same input ----------------------------------------------------
@pytest.mark.parametrize('E', vb.E_LIST)
@pytest.mark.parametrize('name,param', ALL)
def test_per_bin_route_and_sweep_route_agree(name, param, E):
    """The same 16 mixtures as one call (per-bin kernel: tabulated polynomial) and as two calls of
    eight (sweep + finalize kernels: the generic series of embed_dev.hpp): two implementations of
    the same step that must agree with each other and with the oracle."""
    c = vb.case(name, param, E, 'float32' if E % 2 else 'float64')
    one = device_fit(c['y'], c['init'], c['saliency'], 1, c['cmin'], c['cmax'])
    halves = [device_fit(c['y'][s], c['init'][s], c['saliency'][s], 1, c['cmin'], c['cmax'])
              for s in (slice(0, 8), slice(8, 16))]
    two = {k: np.concatenate([h[k] for h in halves]) for k in one}
    print(f'LOGIT-SWEEP {name} {param} E={E}: {logit_error(two, c):.2e}')
    assert_close(one, two, STEP, 'per-bin against sweep', affiliation=two['affiliation'])
    assert_close(two, c['model'], STEP, 'sweep against oracle', affiliation=c['affiliation'])
    assert_close(one, c['model'], STEP, 'per-bin against oracle', affiliation=c['affiliation'])
    assert_clamped(two, c)


# ---- c. the generic series beyond its fixture --------------------------------------------------
C_KAPPAS = np.array([500, 960, 976, 977, 1000, 1500, 2000, 5000, 1e4])


@pytest.mark.parametrize('d', [2, 3, 10, 16, 40])
def test_log_norm_and_log_pdf_beyond_the_fixture(d):
    """wave_log_bessel_over_power past kappa = 500, where tests/golden/embed_vmf_log_norm.npz
    stops: blocks of more than 15 terms (x > 976) re-anchor in the log domain.  log_norm at the
    tolerance of test_vmf_log_norm_series_matches_scipy_ive; log_pdf of rows spread over the
    sphere at the same tolerance plus (d + 8) eps kappa: the d roundings of a dot product and a few
    for the unit row, times the concentration."""
    from pb_bss_amd.distribution import VonMisesFisher
    rng = np.random.default_rng(d)
    mean = np.tile(np.ones(d) / np.sqrt(d), (len(C_KAPPAS), 1))
    vmf = VonMisesFisher(mean=mean, concentration=C_KAPPAS)
    want = oe.vmf_log_norm(C_KAPPAS, d)
    got = vmf.log_norm()
    print(f'log_norm d={d}: worst relative error {np.abs(got / want - 1).max():.1e}')
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=2e-12)
    y = rng.standard_normal((1, 70, d))
    lp = vmf.log_pdf(y)
    ref = oe.vmf_log_pdf(y, mean, C_KAPPAS)
    assert lp.shape == ref.shape == (len(C_KAPPAS), 70)
    bound = 1e-12 * np.abs(want) + 2e-12 + (d + 8) * np.finfo(np.float64).eps * C_KAPPAS
    assert (np.abs(lp - ref) <= bound[:, None]).all(), np.abs(lp - ref).max(-1) / bound


def test_trainer_at_five_classes_with_a_cap_of_2000():
    """K = 5 runs on the round-4 per-bin kernel (embed.hip: vmf_bin_em_kernel) with the generic
    series inside its loop; class 0 sits on max_concentration = 2000 in every iteration."""
    from pb_bss_amd.distribution import VMFMMTrainer
    c = vb.case('generic_series', 2000, 12, 'float32', K=5)
    ref, want = vb.fit_reference(c['y'], c['init'], c['saliency'], 3, 1e-10, 2000.0)
    assert (ref['concentration'][:, 0] == 2000).all() and (ref['concentration'][:, 1:] < 100).all()
    model = VMFMMTrainer().fit(np.array(c['y']), initialization=np.array(c['init']), iterations=3,
                               saliency=np.array(c['saliency']), max_concentration=2000)
    got = dict(mean=model.vmf.mean, concentration=model.vmf.concentration, weight=model.weight,
               affiliation=model.predict(np.array(c['y'])))
    assert_close(got, ref, TRAJECTORY, affiliation=want)
    assert (got['concentration'][:, 0] == 2000).all()


# ---- d. every compiled shape -------------------------------------------------------------------
SHAPE_N = {4: 70, 8: 330}   # NW = 4: two chunks, ragged, two idle waves; NW = 8: six, two idle
SHAPE_P = 10


@functools.lru_cache(maxsize=None)
def shape_case(K, E, dtype, N, uniform):
    """`mild` data with ten probes among the N rows, and the oracle's three-iteration result."""
    c = vb.case('mild', 0, E, dtype, K=K, N=N - SHAPE_P, P=SHAPE_P)
    kw = dict(weight_constant_axis=-2) if uniform else {}
    ref, want = vb.fit_reference(c['y'], c['init'], c['saliency'], 3, 1e-10, 500.0, **kw)
    for a in (*ref.values(), want):
        a.setflags(write=False)
    return c, kw, ref, want


@pytest.mark.parametrize('NW', [4, 8])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('E', [3, 4, 7, 8, 11, 12, 13, 16])
@pytest.mark.parametrize('K', [2, 3, 4])
def test_every_compiled_shape(K, E, dtype, NW, monkeypatch):
    """K in 2..4 x padded feature counts 4, 8, 12, 16 (E on and below the padding) x float32 /
    float64 rows x 4 / 8 wavefronts (pinned; the launcher reads PBBSS_VMF_NW on every call), with
    wavefronts that own no chunk, a ragged last chunk, saliency and, alternating, uniform weights:
    fitted model, predict of that model (the iterations = 0 route) and fit_predict against the
    oracle.  K = 4 with E >= 13 needs 68 accumulators: the kernel refuses it and the round-4
    kernel must serve it."""
    from pb_bss_amd.distribution import VMFMMTrainer
    monkeypatch.setenv('PBBSS_VMF_NW', str(NW))
    uniform = (K + E) % 2 == 1
    c, kw, ref, want = shape_case(K, E, dtype, SHAPE_N[NW], uniform)
    y, init, sal = np.array(c['y']), np.array(c['init']), np.array(c['saliency'])
    model = VMFMMTrainer().fit(y, initialization=init, iterations=3, saliency=sal, **kw)
    got = dict(mean=model.vmf.mean, concentration=model.vmf.concentration, weight=model.weight,
               affiliation=model.predict(y))
    assert_close(got, ref, TRAJECTORY, affiliation=want, weight=not uniform)
    both = VMFMMTrainer().fit_predict(y, initialization=init, iterations=3, saliency=sal, **kw)
    np.testing.assert_allclose(both, want, rtol=0, atol=TRAJECTORY['aff'])
    p = want[:, 0, -SHAPE_P:]
    assert ((p > 0.01) & (p < 0.99)).mean() > 0.5   # the comparison is not of saturated zeros


@pytest.mark.parametrize('K,E,dtype', [(2, 12, 'float32'), (3, 7, 'float64'), (4, 12, 'float32')])
def test_four_and_eight_wavefronts_agree(K, E, dtype, monkeypatch):
    """Identical input with four and with eight wavefronts: only the order of the partial sums
    differs (six chunks on 4 x 2 or 6 x 1 waves), the models agree to 1e-12."""
    c, kw, ref, want = shape_case(K, E, dtype, 330, False)
    out = {}
    for NW in (4, 8):
        monkeypatch.setenv('PBBSS_VMF_NW', str(NW))
        out[NW] = device_fit(c['y'], c['init'], c['saliency'], 3)
    for key in ('mean', 'weight'):
        np.testing.assert_allclose(out[4][key], out[8][key], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out[4]['concentration'], out[8]['concentration'], rtol=1e-12)
    assert_close(out[8], ref, TRAJECTORY, affiliation=want)


# ---- e. route boundaries (results only) --------------------------------------------------------
def test_fifteen_and_sixteen_mixtures():
    """B = 16 is the smallest batch on the per-bin route, B = 15 takes the sweeps."""
    c, kw, ref, want = shape_case(3, 12, 'float32', 330, False)
    big = device_fit(c['y'], c['init'], c['saliency'], 3)
    small = device_fit(c['y'][:15], c['init'][:15], c['saliency'][:15], 3)
    assert_close(big, ref, TRAJECTORY, affiliation=want)
    assert_close(small, {k: v[:15] for k, v in ref.items()}, TRAJECTORY, affiliation=want[:15])
    assert_close({k: v[:15] for k, v in big.items()}, small, TRAJECTORY,
                 affiliation=small['affiliation'])


@pytest.mark.parametrize('K,E', [(1, 12), (5, 12), (2, 17), (4, 17)])
def test_class_and_feature_counts_outside_the_new_kernel(K, E):
    """K = 1, K >= 5 and E > 16 at B = 16: refused by vmf_bin_em2_kernel, served by the round-4
    kernel -- same oracle, same tolerances."""
    c = vb.case('mild', 0, E, 'float32', K=K, N=190, P=10 if K > 1 else 0)
    ref, want = vb.fit_reference(c['y'], c['init'], c['saliency'], 3, 1e-10, 500.0)
    got = device_fit(c['y'], c['init'], c['saliency'], 3)
    assert_close(got, ref, TRAJECTORY, affiliation=want)


def _lds_new(N, K, E, item, NW):
    """VmfBin::lds_bytes (csrc/vmf_bin.hip)."""
    EP = (E + 3) & ~3
    nacc = (K * EP + K + 15) // 16 * 16
    rows = (N + 63) // 64 * 64
    return rows * EP * item + (2 * rows + K * 16 + NW * nacc + 3 * K + 16 * 64) * 8


def _lds_old(N, K, E, item):
    """vmf_bin_lds_bytes (csrc/embed.hip)."""
    KW, ES, S = (K + 1) & ~1, E | 1, 256 // E
    return (N * KW + S * K * E + 4 * K + K * E + K * (E + 1) + 3 * K) * 8 + N * ES * item + 16


def test_rows_beyond_the_new_kernels_lds_budget():
    """E = 2, K = 2, float32: the new kernel pads the two features to four and keeps 1 / |y| and
    the saliency per row (32 bytes a row), the round-4 kernel needs 28.  With the whole LDS of a
    compute unit as the limit (csrc/handle.hip; 160 KiB on gfx950) there are row counts the new
    kernel refuses and the old one takes.  Largest N of the new kernel, one in the gap, largest N
    of the old kernel, and one more (sweeps)."""
    import torch
    limit = max(torch.cuda.get_device_properties(0).shared_memory_per_block, 160 * 1024)
    new_max = max(n for n in range(64, 8192, 64) if _lds_new(n, 2, 2, 4, 8) <= limit)
    old_max = max(n for n in range(64, 8192) if _lds_old(n, 2, 2, 4) <= limit)
    assert new_max + 64 < old_max, (limit, new_max, old_max)
    for N in (new_max, (new_max + old_max) // 2, old_max, old_max + 1):
        c = vb.case('mild', 0, 2, 'float32', N=N - 16, P=16)
        got = device_fit(c['y'], c['init'], c['saliency'], 1)
        print(f'LOGIT lds N={N}: {logit_error(got, c):.2e}')
        assert_close(got, c['model'], STEP, f'N={N}', affiliation=c['affiliation'])


@pytest.mark.parametrize('N', [63, 64, 65, 256, 257])
def test_row_counts_around_the_chunk_size(N):
    c = vb.case('mild', 0, 12, 'float64', K=3, N=N - 6, P=6)
    ref, want = vb.fit_reference(c['y'], c['init'], c['saliency'], 3, 1e-10, 500.0)
    got = device_fit(c['y'], c['init'], c['saliency'], 3)
    assert_close(got, ref, TRAJECTORY, f'N={N}', affiliation=want)


def test_a_single_row():
    """N = 1, K = 3 with the one-hot initialisation: class 0 holds one row, so its mean
    resultant length is 1 +- rounding and eq. 4.4 gives +-1e16 or inf -- one of the two clamps in
    any implementation; classes 1 and 2 are empty.  Mean, weights and the NaN pattern of the
    oracle; the concentration of class 0 on a clamp.  (Where the length is 1 exactly the
    reference has (E - 1) / 0 = inf -> the cap; the kernel's Newton reciprocal made NaN of it in
    8 of these 16 mixtures until vmf_bin.hip selected around the zero denominator.)"""
    y, init, sal = vb.scenario(12, 3, 1, 0.1, 5, np.float32)
    with np.errstate(all='ignore'):
        ref, want = vb.fit_reference(y, init, sal, 1, 1e-10, 500.0)
    got = device_fit(y, init, sal, 1)
    np.testing.assert_allclose(got['mean'], ref['mean'], rtol=0, atol=1e-9)
    np.testing.assert_allclose(got['weight'], ref['weight'], rtol=0, atol=1e-10)
    assert np.isin(got['concentration'][:, 0], (1e-10, 500.0)).all(), got['concentration'][:, 0]
    assert np.isnan(ref['concentration'][:, 1:]).all() and np.isnan(want).all()
    assert np.isnan(got['concentration'][:, 1:]).all() and np.isnan(got['affiliation']).all()


# ---- f. edge rows and isolation ----------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_an_all_zero_row(dtype):
    """The reference divides a zero row by `tiny`: it stays zero, every dot product is 0 and its
    posterior is weight_k exp(offset_k) normalised -- the normaliser and nothing else."""
    c = vb.case('mild', 0, 12, dtype, K=3)
    y = np.array(c['y'])
    y[::2, 7] = 0
    y[1::2, -1] = 0   # a probe row (saliency 0)
    ref, want = vb.fit_reference(y, c['init'], c['saliency'], 1, 1e-10, 500.0)
    assert np.isfinite(want).all() and (want[::2, :, 7] > 1e-3).all()
    got = device_fit(y, c['init'], c['saliency'], 1)
    assert_close(got, ref, STEP, affiliation=want)


@pytest.mark.parametrize('dtype,power', [('float64', 400), ('float32', 60)])
def test_rows_scaled_by_powers_of_two(dtype, power):
    """Scaling a row by a power of two is exact and the model only sees y / |y|: masks and model of
    a call whose mixture 3 has its rows scaled by 2^+-power are bit-identical to the unscaled
    call's (|y|^2 stays normal: 2^-800 in float64, 2^-120 accumulated in float64 for float32)."""
    c = vb.case('clamped_high', 500, 12, dtype)
    y = np.array(c['y'])
    plain = device_fit(y, c['init'], c['saliency'], 2)
    scale = np.where(np.arange(y.shape[1]) % 2 == 0, 2.0 ** power, 2.0 ** -power).astype(y.dtype)
    y[3] *= scale[:, None]
    assert np.isfinite(y).all() and (np.abs(y[3]).max(-1) > 0).all()
    scaled = device_fit(y, c['init'], c['saliency'], 2)
    for key in plain:
        assert np.array_equal(plain[key], scaled[key]), key


def test_an_empty_class_poisons_its_own_mixture_only():
    """Class 1 of mixture 5 starts exactly at zero: 0 / 0 in its mean resultant length.  NaN where
    the oracle has NaN (its concentration, every posterior of that mixture), finite values where
    the oracle has them (mean 0 / tiny = 0, weights 1 and 0); the other fifteen mixtures are
    bit-identical to a call in which mixture 5 is an ordinary one."""
    c = vb.case('mild', 0, 12, 'float32')
    init = np.array(c['init'])
    plain = device_fit(c['y'], init, c['saliency'], 2)
    init[5, 0], init[5, 1] = 1.0, 0.0
    with np.errstate(all='ignore'):
        ref, want = vb.fit_reference(c['y'], init, c['saliency'], 1, 1e-10, 500.0)
    assert np.isnan(ref['concentration'][5, 1]) and np.isnan(want[5]).all()
    assert np.isfinite(want[np.arange(vb.B) != 5]).all() and (ref['mean'][5, 1] == 0).all()
    got = device_fit(c['y'], init, c['saliency'], 1)
    assert_close(got, ref, STEP, affiliation=want)   # assert_allclose: NaN only where ref has NaN
    poisoned = device_fit(c['y'], init, c['saliency'], 2)
    keep = np.arange(vb.B) != 5
    for key in plain:
        assert np.array_equal(plain[key][keep], poisoned[key][keep]), key
    assert np.isnan(poisoned['affiliation'][5]).all()


# ---- g. min_concentration of 0 and of a denormal -----------------------------------------------
@pytest.mark.parametrize('cmin', [0.0, 5e-324])
@pytest.mark.parametrize('cmax', [10.0, 500.0])
def test_floor_of_zero_or_a_denormal(cmin, cmax):
    """A class whose resultant is exactly 0 (rows +-e_j, dyadic affiliations: nothing rounds) gets
    the concentration min_concentration; at 0 or a denormal the normaliser is the limit
    -nu ln 2 - ln Gamma(nu + 1) of ln(I_nu(x) / x^nu), which the generic series reaches through
    IEEE log(0) = -inf.  The tabulated polynomial takes ln x from a series that is valid for
    normal numbers only: before vmf_bin.hip left that path to min_concentration >= tiny its
    spurious terms moved these posteriors by 1.26e-6 (5e-6 in the offset) at max_concentration = 10
    and a floor of 0 (one term per lane), and by nothing at 500 (nine terms: e^-100) or at a
    denormal (frexp is right there).  The per-bin route (B = 16) must agree with the sweep
    route (B = 8 twice), NaN for NaN and to 1e-9 otherwise -- and both with the oracle at a floor
    of 1e-300, where its own formula is still finite and 1e-300 from the limit."""
    y, init = vb.edge_rows(4)
    one = device_fit(y, init, None, 1, cmin, cmax)
    halves = [device_fit(y[s], init[s], None, 1, cmin, cmax) for s in (slice(0, 8), slice(8, 16))]
    two = {k: np.concatenate([h[k] for h in halves]) for k in one}
    sal = np.ones(y.shape[:2])
    ref, want = vb.fit_reference(y, init, sal, 1, 1e-300, cmax)
    assert (ref['concentration'][:, 1] == 1e-300).all() and np.isfinite(want).all()
    assert (np.abs(want[:, 0, :2] - 0.5) < 0.45).all()   # rows +-e_0: decided by the offsets
    print(f'floor {cmin} cap {cmax}: per-bin against sweep '
          f"{np.nanmax(np.abs(one['affiliation'] - two['affiliation'])):.2e}, per-bin against the "
          f"limit {np.nanmax(np.abs(one['affiliation'] - want)):.2e}, sweep against the limit "
          f"{np.nanmax(np.abs(two['affiliation'] - want)):.2e}")
    assert (one['concentration'][:, 1] == cmin).all() and (two['concentration'][:, 1] == cmin).all()
    for key in ('mean', 'concentration', 'weight', 'affiliation'):
        np.testing.assert_allclose(one[key], two[key], rtol=0, atol=1e-9, err_msg=key)
    for got in (one, two):
        np.testing.assert_allclose(got['mean'], ref['mean'], rtol=0, atol=1e-9)
        np.testing.assert_allclose(got['concentration'][:, 0], ref['concentration'][:, 0], rtol=1e-8)
        np.testing.assert_allclose(got['affiliation'], want, rtol=0, atol=1e-9)
