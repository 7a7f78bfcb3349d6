"""GPU: the warm-started eigenpair of the complex-Watson M-step on hard spectra.

From the second EM iteration of a launch on the kernel (csrc/cwmm.hpp: factor_class) takes each
class's dominant eigenpair from a shifted inverse iteration started at the previous mode
(csrc/wave_la.hpp: wave_dominant_eigenpair): accepted at a residual of 1e-12 trace, certified
dominant by the sign of the pivots of sigma I - C, with the cyclic Jacobi as the fall-back.  The
other Watson tests draw well-separated sources (eigengap ~ 0.1, a mode that moves a little per
iteration); here the inputs come from tests/oracle_watson_spectra.py, whose promises
tests/test_watson_spectra_oracle.py asserts on the CPU: two leading eigenvalues g apart
(g = 1e-1 .. 1e-9, 0), a mode that jumps to an orthogonal vector between two iterations (the warm
start is then an exact eigenvector of the new covariance, of its SECOND eigenvalue), an isotropic
class, a rank-one class, a class without mass.

The device A/B (`ab`): the same arithmetic feeds both eigensolvers.
    L1  gamma0 = init, n iterations                -> M[n-1]
    L2  model = M[n-1], 1 iteration                -> E-step, then Jacobi (the first iteration of
                                                      a launch is never warm)   -> M[n] "jacobi"
    L3  gamma0 = init, n + 1 iterations            -> iteration n warm-started  -> M[n] "warm"
n = 1, or the iteration of the jump.  Both M[n] are judged on C = covariance_after(M[n-1] of the
DEVICE, Y) in float64, so that a legitimate choice of M[n-1] inside a degenerate eigenspace does
not leak into the comparison.  That iteration n - 1 of L3 equals L1 cannot be observed (a launch
returns its last model only); the fallback of the issue is asserted instead: L1 is
bit-reproducible across two calls.

Bounds (none taken from the device):
  concentration   |warm - jacobi|, and each against spline(lambda_max(C)): slope of the oracle
                  spline at lambda_max (finite difference) x 1e-11 trace, ten times the accepted
                  residual; trace = 1.  Outside the spline's range (isotropic, rank one) the slope
                  is 0: the values are equal.
  cluster         the smallest set of leading eigenvalues of C that is >= 0.05 above the rest
                  (asserted to be the pair, at most max(10 g, 1e-8) wide, for near_degenerate);
                  the part of the device mode outside its eigenspace is <= 1e-8 = (1e-12 accepted
                  residual + 1e-9 device-vs-float64 covariance, tests/test_gpu_em.py) / sep,
                  rounded down; Rayleigh quotient >= lambda_max - (width + 1e-9).
  dominance       where the leading eigenvalue is >= 1e-4 above the second, overlap with its
                  eigenvector >= 1 - 1e-10 (test_cwmm_trainer_matches_reference's); at the jump
                  also overlap with M[n-1] < 0.5: a certificate that accepts the stale vector
                  fails both.
Whole trajectories (4 iterations, affiliation < 1e-7, concentration < 1e-8 max: the tolerances of
tests/test_gpu_cwmm.py) are compared where the oracle's own error is < 1e-9 (CPU test): g = 1e-1,
1e-3 at D = 4, 6, 8; g = 1e-5 at D = 7, 8 only -- EM amplifies a rotation inside the
near-degenerate plane, at D = 4, 5, 6 the float64 reference differs from itself by 8e-4, 1e-5,
1e-7 -- and every mode_jump.  For g = 1e-6, 1e-9, 0 only the A/B applies: trajectories may
legitimately differ.

Measured on an MI355X (largest over the parametrisation; every test prints its own with -s):
  |kappa warm - jacobi|           6.1e-13   bound >= 1.6e-10 (near_degenerate 1.2e-13,
  |kappa - spline(lambda_max)|    8.0e-13                    mode_jump 6.1e-13, split 1.6e-13)
  outside the cluster             1.4e-12   bound 1e-8
  Rayleigh deficit beyond width   6.7e-16   bound 1e-9
  overlap with the stale mode     1.1e-14   bound 0.5
  affiliation, 4 iterations       g = 1e-1: 7.8e-16; 1e-3: 3.4e-11 (D = 4); 1e-5: 1.2e-9 (D = 7,
                                  T = 320; 2.0e-10 at T = 192; D = 8: 1.8e-12); mode_jump 6.7e-16;
                                  split groups 1.4e-15; shared weights 1.6e-15   bound 1e-7
  concentration / max             2.2e-14   bound 1e-8
Mutations of wave_dominant_eigenpair (not kept; each run once): accepting at the first residual
test without the certificate fails every mode_jump case here but the complex64 one (61 tests,
affiliations off by 2e-4 .. 2e-2; in complex64 the stale vector is 1e-8 off an eigenvector and
is not accepted at once); an acceptance tolerance of 1e-9 trace fails the concentration bound of
near_degenerate(1e-9) (|kappa warm - jacobi| 2.9e-10 .. 1.4e-8 against 1.9e-10 .. 2.8e-10).
"""
import functools

import numpy as np
import pytest

import oracle_watson_spectra as ws

pytestmark = pytest.mark.gpu

TS = (192, 320)  # four-wave kernel; eight-wave kernel (T > 256 and a compute unit per bin)
SEP = 0.05


@functools.lru_cache(maxsize=None)
def splines(D):
    """(device spline of the kernel, the oracle's scipy spline) for D sensors"""
    from pb_bss_amd.distribution import ComplexWatsonTrainer
    from oracle import cwmm as ow
    return ComplexWatsonTrainer(D).device_spline(), ow.make_spline(D)


def fit(Y, *, init=None, model=None, iterations, **kw):
    """engine.cwmm_fit on numpy arrays -> dict of numpy arrays (None entries dropped)"""
    from pb_bss_amd import _lib, engine
    t = _lib.torch()
    y = _lib.to_device(Y)
    D = Y.shape[-1]
    if model is not None:
        K = model['mode'].shape[1]
        w = np.broadcast_to(model['weight'].reshape(-1, K), model['concentration'].shape)
        kw['model'] = (_lib.to_device(model['mode'], t.complex128),
                       _lib.to_device(model['concentration'], t.float64),
                       _lib.to_device(w, t.float64))
    else:
        K = init.shape[1]
        kw['gamma0'] = _lib.to_device(init, t.float64)
    r = engine.cwmm_fit(y, K, splines(D)[0], iterations=iterations, **kw)
    assert r is not None, 'the cooperative kernel did not serve the launch'
    return {k: _lib.to_host(v) for k, v in r.items() if v is not None}


def oracle_model(r):
    """device result -> the model dict of oracle.cwmm (weight (F, K, 1) or (1, K, 1))"""
    return dict(mode=r['mode'], concentration=r['concentration'], weight=r['weight'][..., None])


def ab(Y, init, n=1, **kw):
    """The three launches of the module docstring.  kw: weight_mode / group of L1 and L3."""
    Y128 = Y.astype(np.complex128)
    prev = fit(Y, init=init, iterations=n, **kw)
    again = fit(Y, init=init, iterations=n, **kw)
    for key in ('mode', 'concentration', 'weight'):
        assert np.array_equal(prev[key], again[key]), key  # L1 is bit-reproducible
    jacobi = fit(Y, model=prev, iterations=1)
    warm = fit(Y, init=init, iterations=n + 1, **kw)
    for r in (prev, jacobi, warm):
        assert (r['status'] == 0).all(), r['status']
    cov = ws.covariance_after(oracle_model(prev), Y128)
    return dict(prev=prev, jacobi=jacobi, warm=warm, cov=cov)


def cluster_of(val):
    """ascending eigenvalues -> (n, width, sep) of the smallest leading set >= SEP above the rest"""
    D = len(val)
    for n in range(1, D):
        if val[-n] - val[-n - 1] >= SEP:
            return n, float(val[-1] - val[-n]), float(val[-n] - val[-n - 1])
    return D, float(val[-1] - val[0]), np.inf


def check_ab(res, what, classes=None):
    """Every assertion of the module docstring that needs no knowledge of the scenario; returns
    the measured figures, largest over bins and classes, and the clusters found."""
    cov = res['cov']
    F, K, D, _ = cov.shape
    spline = splines(D)[1]
    fig = dict(conc_ab=0.0, conc_ref=0.0, conc_bound=np.inf, outside=0.0, rayleigh=-np.inf)
    clusters = {}
    for f in range(F):
        for k in range(K) if classes is None else classes:
            val, vec = np.linalg.eigh(cov[f, k])
            n, width, sep = cluster_of(val)
            clusters[f, k] = (n, width, sep, float(val[-1] - val[-2]))
            ref = float(spline(val[-1]))
            bound = ws.spline_slope(spline, val[-1]) * 1e-11
            cw, cj = (float(res[p]['concentration'][f, k]) for p in ('warm', 'jacobi'))
            fig['conc_ab'] = max(fig['conc_ab'], abs(cw - cj))
            fig['conc_ref'] = max(fig['conc_ref'], abs(cw - ref), abs(cj - ref))
            fig['conc_bound'] = min(fig['conc_bound'], bound)
            assert abs(cw - cj) <= bound, (what, f, k, cw, cj, bound)
            assert abs(cw - ref) <= bound and abs(cj - ref) <= bound, (what, f, k, cw, cj, ref, bound)
            for p in ('warm', 'jacobi'):
                m = res[p]['mode'][f, k]
                assert np.isfinite(m).all() and abs(np.linalg.norm(m) - 1) < 1e-12, (what, p, f, k)
                if n < D:
                    out = ws.outside_cluster(m, vec, n)
                    fig['outside'] = max(fig['outside'], out)
                    assert out <= 1e-8, (what, p, f, k, out, n, sep)
                deficit = val[-1] - ws.rayleigh(m, cov[f, k])
                fig['rayleigh'] = max(fig['rayleigh'], deficit - width)
                assert deficit <= width + 1e-9, (what, p, f, k, deficit, width)
                if val[-1] - val[-2] >= 1e-4:
                    ov = ws.overlap(m, vec[:, -1])
                    assert ov >= 1 - 1e-10, (what, p, f, k, ov)
    print(f'{what}: |kappa warm - jacobi| {fig["conc_ab"]:.1e}, |kappa - spline| '
          f'{fig["conc_ref"]:.1e} (smallest bound {fig["conc_bound"]:.1e}); outside the cluster '
          f'{fig["outside"]:.1e}; Rayleigh deficit beyond the width {fig["rayleigh"]:.1e}')
    return fig, clusters


def check_parity(Y, init, what, tr=None, **kw):
    """One launch of 4 iterations with final_predict against the oracle's trajectory."""
    from oracle import cwmm as ow
    Y128 = Y.astype(np.complex128)
    shared = 'weight_mode' in kw
    if tr is None:
        tr = ws.trajectory(Y128, init, 4, weight_constant_axis=(-3, -1) if shared else (-1,))
    want = tr[-1]
    r = fit(Y, init=init, iterations=4, final_predict=True, **kw)
    assert (r['status'] == 0).all(), r['status']
    e_aff = np.abs(r['affiliation'] - ow.cwmm_predict(want, Y128)).max()
    e_conc = np.abs(r['concentration'] - want['concentration']).max() / want['concentration'].max()
    e_w = np.abs(r['weight'][..., None] - want['weight']).max()
    print(f'{what}: affiliation {e_aff:.1e}, concentration / max {e_conc:.1e}, weight {e_w:.1e}')
    assert e_aff < 1e-7 and e_conc < 1e-8 and e_w < 1e-9, (what, e_aff, e_conc, e_w)
    return r, tr


def near_degenerate_structure(clusters, g, what):
    """Class 0 of C is what the scenario promises (the device's own M[n-1] went into C)."""
    for (f, k), (n, width, sep, gap) in clusters.items():
        if k != 0:
            continue
        assert sep >= SEP, (what, f, n, sep)
        if g >= 5e-3:
            assert n == 1, (what, f, n)  # one leading eigenvalue, >= 0.05 above the second
        elif g > 0:
            assert n == 2 and width <= max(10 * g, 1e-8), (what, f, n, width)
        else:
            assert n <= 2, (what, f, n)  # the E-step has split the degenerate pair (CPU test)


AB_NEAR_DEGENERATE = sorted({(g, D) for g in ws.GAPS for D in (4, 6, 8)} |
                            {(1e-5, D) for D in ws.NEAR_DEGENERATE_D})


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('g,D', AB_NEAR_DEGENERATE)
def test_warm_start_equals_jacobi_on_a_near_degenerate_pair(g, D, T):
    """near_degenerate(g), A/B at iteration 1: the leading pair of class 0 is 0.9 g .. 1.0 g apart
    and >= 0.2 above the rest.  Every sensor count with a kernel of its own at g = 1e-5 (D = 2, 3
    cannot carry the scenario, see oracle_watson_spectra.DROPPED), D = 4, 6, 8 otherwise."""
    Y, init, _ = ws.near_degenerate(g, D=D, F=3, T=T, iterations=1)
    what = f'near_degenerate g={g:g} D={D} T={T}'
    _, clusters = check_ab(ab(Y, init), what)
    near_degenerate_structure(clusters, g, what)


AB_MODE_JUMP = sorted({(s, D) for s in ws.SHARES for D in (3, 6, 8)} |
                      {(0.3, D) for D in ws.MODE_JUMP_D})


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('share,D', AB_MODE_JUMP)
def test_warm_start_follows_a_mode_jump(share, D, T):
    """mode_jump(share), A/B at the iteration of the jump (1 at D >= 6; 1 or 2 below): the previous
    mode is an eigenvector of the new covariance, of its second eigenvalue, 0.003 .. 0.06 below
    the first.  Warm and Jacobi both return the new leading eigenvector (overlap >= 1 - 1e-10) and
    not the stale one (overlap with M[n-1] < 0.5; 1e-14 in the oracle)."""
    Y, init, p = ws.mode_jump(share, D=D, F=3, T=T)
    n = p['jump_at']
    what = f'mode_jump share={share} D={D} T={T} (iteration {n})'
    res = ab(Y, init, n)
    _, clusters = check_ab(res, what)
    stale = 0.0
    for f in range(Y.shape[0]):
        ncl, width, sep, gap = clusters[f, 0]
        assert ncl <= 2 and sep >= SEP and gap >= 1e-3, (what, f, clusters[f, 0])
        lead = np.linalg.eigh(res['cov'][f, 0])[1][:, -1]
        for path in ('warm', 'jacobi'):
            m = res[path]['mode'][f, 0]
            assert ws.overlap(m, lead) >= 1 - 1e-10, (what, path, f)
            stale = max(stale, ws.overlap(m, res['prev']['mode'][f, 0]))
            assert ws.overlap(m, res['prev']['mode'][f, 0]) < 0.5, (what, path, f)
    print(f'{what}: largest overlap with the stale mode {stale:.1e}')


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('D', [2, 3, 6, 8])
def test_warm_start_on_an_isotropic_and_a_rank_one_class(D, T):
    """One class (the affiliation is 1: the same covariance at every iteration, the warm start an
    exact eigenvector).  isotropic: every vector is dominant -- unit norm, finite, concentration 0
    on both paths.  rank_one (lam_2 = 1e-12 in the even bins, exactly 0 in the odd ones):
    sigma I - C is singular to 1e-10 in one direction; the mode is the block's leading vector and
    the concentration sits at the cap, equal on both paths."""
    Y, init, _ = ws.isotropic(D=D, F=3, T=T, iterations=1)
    res = ab(Y, init)
    _, clusters = check_ab(res, f'isotropic D={D} T={T}')
    assert all(c[0] == D for c in clusters.values()), clusters
    for path in ('warm', 'jacobi'):
        assert (res[path]['concentration'] == 0).all(), res[path]['concentration']
    Y, init, _ = ws.rank_one(D=D, F=4, T=T, iterations=1)
    res = ab(Y, init)
    _, clusters = check_ab(res, f'rank_one D={D} T={T}')
    assert all(c[0] == 1 for c in clusters.values()), clusters
    for path in ('warm', 'jacobi'):
        assert (res[path]['concentration'] == 500).all(), res[path]['concentration']


PARITY = ([('near_degenerate', g, D) for g, D in ws.PARITY_NEAR_DEGENERATE] +
          [('mode_jump', s, D) for s, D in ws.PARITY_MODE_JUMP])


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('kind,x,D', PARITY)
def test_trajectory_matches_the_oracle(kind, x, D, T):
    """4 iterations in one launch (three of them warm) against the oracle at the tolerances of
    tests/test_gpu_cwmm.py, wherever the oracle's own error is below 1e-9 (module docstring).
    At g = 1e-5 an eigenvector accepted AT the residual tolerance would be 1e-12 / 1e-5 = 1e-7
    off inside the pair's plane."""
    Y, init, p = getattr(ws, kind)(x, D=D, F=3, T=T)
    what = f'{kind}({x:g}) D={D} T={T}'
    r, tr = check_parity(Y, init, what, tr=p['trajectory'])
    if kind == 'mode_jump':
        ov = ws.overlap(r['mode'], tr[-1]['mode'])
        assert (ov >= 1 - 1e-10).all(), (what, ov)


@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('D', [3, 6, 8])
def test_a_class_without_mass(D, T):
    """In bin 1 of 4 class 1 of the initialisation is exactly zero: its covariance is 0 / 0 at
    every iteration (its weight is 0, so it never gains a frame).  ST_NONFINITE is set for that
    (bin, class) pair, no other bit in that bin (the reference's NaN would also reach the bin's
    other class; the device reports through the status word and lets class 0 carry on alone:
    measured status [[0, 0], [0, 1], [0, 0], [0, 0]]), nothing in any other bin, and the other
    bins equal (1e-9) a launch without that bin and (1e-7) the oracle."""
    from pb_bss_amd import _lib
    from oracle import cwmm as ow
    Y, init, p = ws.empty_class(D=D, F=4, T=T, iterations=3)
    e, keep = p['empty_bin'], p['keep']
    r = fit(Y, init=init, iterations=3, final_predict=True, check_status=False)
    assert r['status'][e, 1] & _lib.ST_NONFINITE, r['status']
    assert ((r['status'][e] | _lib.ST_NONFINITE) == _lib.ST_NONFINITE).all(), r['status']
    assert (r['status'][keep] == 0).all(), r['status']
    from pb_bss_amd.engine import StatusAssertionError
    with pytest.raises(StatusAssertionError):  # by default the status word becomes the reference's
        fit(Y, init=init, iterations=3)  # `assert np.isfinite(...)`
    alone = fit(Y[keep], init=init[keep], iterations=3, final_predict=True)
    assert (alone['status'] == 0).all()
    assert np.abs(r['affiliation'][keep] - alone['affiliation']).max() <= 1e-9
    assert np.abs(r['concentration'][keep] - alone['concentration']).max() <= 1e-9
    assert np.abs(r['weight'][keep] - alone['weight']).max() <= 1e-9
    assert (ws.overlap(r['mode'][keep], alone['mode']) >= 1 - 1e-9).all()
    want = ow.cwmm_predict(p['trajectory'][-1], Y[keep])
    assert np.abs(alone['affiliation'] - want).max() < 1e-7


@pytest.mark.parametrize('kind,x', [('near_degenerate', 1e-3), ('mode_jump', 0.3)])
def test_split_groups_on_hard_spectra(kind, x):
    """257 bins for 256 compute units, T = 320, complex64 input (the oracle is fed the exact
    upcast): bin 256 runs as split groups on the side stream (csrc/cwmm.hpp: WatsonSplit, from
    three iterations on), bin 0 in the main launch.  Both hold the same scenario bin, the others
    ordinary data.  The two copies agree at 1e-9 (test_cwmm_remainder_bins_as_split_groups), both
    match the oracle after 4 iterations, and both pass the A/B at the last iteration: 3
    iterations -> M[2], 4 iterations -> M[3] warm, model = M[2] -> M[3] by Jacobi."""
    from pb_bss_amd import engine
    from oracle import synth
    F, T, D, K = 257, 320, 6, 2
    Y, init = synth.make_stft(F, T, D, K, seed=7)
    assert Y.dtype == np.complex64
    Yb, initb, _ = getattr(ws, kind)(x, D=D, F=1, T=T, iterations=1)
    Y, init = Y.copy(), init.copy()
    Y[0] = Y[256] = Yb[0].astype(np.complex64)
    init[0] = init[256] = initb[0]
    two = [0, 256]
    was = engine.split_tail()
    try:
        engine.set_split_tail(1)
        res = ab(Y, init, 3)
        full = fit(Y, init=init, iterations=4, final_predict=True)
    finally:
        engine.set_split_tail(was)
    sub = dict(cov=res['cov'][two], **{p: {k: v[two] for k, v in res[p].items()}
                                       for p in ('prev', 'jacobi', 'warm')})
    what = f'split groups, {kind}({x:g})'
    check_ab(sub, what)
    for key in ('affiliation', 'concentration', 'weight'):
        assert np.abs(full[key][0] - full[key][256]).max() <= 1e-9, key
    assert (ws.overlap(full['mode'][0], full['mode'][256]) >= 1 - 1e-9).all()
    from oracle import cwmm as ow
    Y2 = Y[two].astype(np.complex128)
    tr = ws.trajectory(Y2, init[two], 4)
    assert ws.self_spread(Y2[:1], init[:1], 4)[0] < 1e-9  # the comparison is well posed
    e_aff = np.abs(full['affiliation'][two] - ow.cwmm_predict(tr[-1], Y2)).max()
    e_conc = np.abs(full['concentration'][two] - tr[-1]['concentration']).max()
    print(f'{what}: affiliation {e_aff:.1e}, concentration {e_conc:.1e}')
    assert e_aff < 1e-7 and e_conc < 1e-8 * tr[-1]['concentration'].max()


@pytest.mark.parametrize('kind,x', [('near_degenerate', 1e-3), ('mode_jump', 0.3)])
def test_cooperative_shared_weight_kernel_on_hard_spectra(kind, x):
    """weight_constant_axis (-3, -1): one weight set for the F = 5 bins, the cooperative kernel
    (csrc/cwmm.hpp: WatsonShared) runs the same factor_class.  Against the oracle's trajectory
    with shared weights, and the A/B at iteration 1 (the Jacobi launch is the ordinary kernel fed
    the shared weights: the M-step does not depend on how the weights were averaged)."""
    from pb_bss_amd import _lib
    F, D, T = 5, 6, 192
    Y, init, _ = getattr(ws, kind)(x, D=D, F=F, T=T, iterations=1)
    kw = dict(weight_mode=_lib.WEIGHT_SHARED_K, group=F)
    what = f'shared weights, {kind}({x:g})'
    r, tr = check_parity(Y, init, what, **kw)
    assert r['weight'].shape == (1, 2)
    jumps = [i for i in range(1, 4) if
             ws.overlap(tr[i - 1]['mode'][:, 0], tr[i]['mode'][:, 0]).max() < 0.5]
    n = jumps[0] if jumps else 1
    assert (kind == 'mode_jump') == bool(jumps), jumps
    res = ab(Y, init, n, **kw)
    check_ab(res, f'{what} (iteration {n})')
    if jumps:
        for path in ('warm', 'jacobi'):
            assert (ws.overlap(res[path]['mode'][:, 0], res['prev']['mode'][:, 0]) < 0.5).all()
