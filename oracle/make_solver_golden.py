"""Recipe of tests/golden/solver_hard_cases.npz: the ill-conditioned and badly scaled inputs of
oracle/solver_cases.py, their solutions in 50-digit arithmetic (mpmath), and the error that LAPACK
(numpy.linalg.eigh / solve, scipy.linalg.eigh(a, b) / eig(a, b)) makes on the same float64 inputs.

    python -m oracle.make_solver_golden            # rewrites the fixture, bit for bit
    python -m oracle.make_solver_golden --check    # rebuilds in memory and compares

Needs mpmath and scipy; the tests need neither (tests/test_solver_golden.py re-derives three cases
where mpmath imports).  Layout (solver_cases.load_fixture): one array per 'solver|family|D|field';
a derived case shares the fields it does not carry with its base (solver_cases.ref).
  heev   a (packed lower triangle) or rule; w (D) eigenvalues ascending; v (D, 2) the two leading
         eigenvectors, principal first; info = [||A||_2, kappa_2, relative gap of the principal
         eigenvalue, relative gap below the leading pair]; lapack = heev_metrics of numpy's eigh
  solve  a, b or rule; x; info = [||A||_2, kappa_2]; lapack = [relative Frobenius error]
  gev    t, n (packed), atf, atf2 or rule; w (N-normalised), lam; info = [kappa_2(N), relative
         gap of lam]; lapack = gev_metrics of scipy eigh(t, n); lapack_eig = those of scipy
         eig(t, n) with ||w|| = 1; the beamformer outputs (mvdr, souden_mat, ...; lcmv up to
         D = 8; above D = 9 wmwf_scale = Re tr G / (1 + tr G) in place of wmwf_mat, which is
         souden_mat times it) and bf_lapack = their relative errors in float64 NumPy
  gevgen the non-Hermitian pencil: w (unit norm), lam (complex), info, lapack_eig
"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np

from oracle import solver_cases as sc

DIGITS = 50
PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden',
                    'solver_hard_cases.npz')


def _mp():
    import mpmath
    mpmath.mp.dps = DIGITS
    return mpmath


def to_mp(a):
    mp = _mp()
    a = np.asarray(a)
    if a.ndim == 1:
        a = a[:, None]
    return mp.matrix([[mp.mpc(float(z.real), float(z.imag)) for z in row] for row in a])


def to_np(m):
    return np.array([[complex(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def mp_heev(a):
    """-> (w, v, info) in float64 from the 50-digit eigendecomposition."""
    mp = _mp()
    E, Q = mp.eighe(to_mp(a))
    D = a.shape[0]
    lam = [E[i] for i in range(D)]
    mags = [abs(x) for x in lam]
    norm2 = max(mags)
    kappa = norm2 / min(mags) if min(mags) > 0 else mp.inf
    gap = (lam[-1] - lam[-2]) / norm2
    gap_pair = (lam[-2] - lam[-3]) / norm2 if D > 2 else mp.mpf(1)
    v = to_np(Q)[:, [D - 1, D - 2]]
    return (np.array([float(x) for x in lam]), v,
            np.array([float(norm2), float(kappa), float(gap), float(gap_pair)]))


def mp_solve(a, b):
    mp = _mp()
    A = to_mp(a)
    s = mp.svd_c(A, compute_uv=False)
    s = [s[i] for i in range(a.shape[0])]
    return to_np(mp.inverse(A) * to_mp(b)), np.array([float(max(s)), float(max(s) / min(s))])


def mp_gev(t, n):
    """Principal pair of T w = lam N w, w^H N w = 1 -> (w, lam, [kappa_2(N), relative gap])."""
    mp = _mp()
    T, N = to_mp(t), to_mp(n)
    D = t.shape[0]
    EN, _ = mp.eighe(N)
    kappa = EN[D - 1] / EN[0]
    L = mp.cholesky(N)
    X = mp.inverse(L)
    E, Q = mp.eighe(X * T * X.H)
    w = X.H * Q[:, D - 1]
    return (to_np(w)[:, 0], float(E[D - 1]),
            np.array([float(kappa), float((E[D - 1] - E[D - 2]) / E[D - 1])]))


def mp_gev_general(t, n):
    """Eigenpair of N^-1 T with the largest eigenvalue by numpy's complex argmax (real part, ties
    by the imaginary part) -> (unit w, lam, [kappa_2(N), relative distance to the next one])."""
    mp = _mp()
    T, N = to_mp(t), to_mp(n)
    D = t.shape[0]
    EN, _ = mp.eighe(N)
    kappa = EN[D - 1] / EN[0]
    E, ER = mp.eig(mp.inverse(N) * T)
    k = max(range(D), key=lambda i: (mp.re(E[i]), mp.im(E[i])))
    w = ER[:, k]
    w = w / mp.norm(w)
    gap = min(abs(E[k] - E[i]) for i in range(D) if i != k) / abs(E[k])
    return to_np(w)[:, 0], complex(E[k]), np.array([float(kappa), float(gap)])


def mp_beamformers(t, n, atf, atf2, w, D):
    """oracle/beamformer.py's mvdr_souden (matrix and the two SNR terms), wmwf, mvdr, ban and lcmv
    on one pencil, in 50 digits."""
    mp = _mp()
    T, N = to_mp(t), to_mp(n)
    Ni = mp.inverse(N)
    G = Ni * T
    tr = sum(G[i, i] for i in range(D))
    mat = G / mp.re(tr)
    TM, NM = T * mat, N * mat
    out = {'souden_mat': to_np(mat),
           'souden_num': np.array([complex(sum(mp.conj(mat[d, r]) * TM[d, r] for d in range(D)))
                                   for r in range(D)]),
           'souden_den': np.array([complex(sum(mp.conj(mat[d, r]) * NM[d, r] for d in range(D)))
                                   for r in range(D)]),
           'wmwf_mat': to_np(G / (1 + tr)),
           'wmwf_scale': np.array(complex(mp.re(tr) / (1 + tr)))}
    a, a2, wv = to_mp(atf), to_mp(atf2), to_mp(w)
    x = mp.inverse((N + N.H) / 2) * a
    out['mvdr'] = to_np(x / (a.H * x)[0, 0])[:, 0]
    nw = N * wv
    nom = mp.sqrt((wv.H * N * nw)[0, 0])
    den = abs((wv.H * nw)[0, 0])
    out['ban'] = to_np(wv * abs(nom / den))[:, 0]
    if D <= sc.LCMV_MAX_D:
        p1, p2 = Ni * a, Ni * a2
        hph = mp.matrix([[(a.H * p1)[0, 0], (a.H * p2)[0, 0]],
                         [(a2.H * p1)[0, 0], (a2.H * p2)[0, 0]]])
        tmp = mp.inverse(hph) * mp.matrix([mp.mpf(float(r)) for r in sc.LCMV_RESPONSE])
        out['lcmv'] = to_np(p1 * tmp[0] + p2 * tmp[1])[:, 0]
    return out


def reference(cases, key):
    """Reference arrays and LAPACK's errors of one case."""
    import scipy.linalg
    solver, fam, D = key.split('|')
    D = int(D)
    x = sc.inputs(cases, key)
    out = {}
    if solver == 'heev':
        rule = str(cases[key].get('rule', ''))
        if rule.startswith('scale:'):  # power of two: the exact answer scales exactly
            base = reference.cache[f'heev|{sc.HEEV_BASE}|{D}']
            s = int(rule[6:])
            out['w'] = np.ldexp(base['w'], s)
            out['info'] = base['info'] * np.array([2.0 ** s, 1.0, 1.0, 1.0])
            v = base['v']
        else:
            out['w'], v, out['info'] = mp_heev(x['a'])
            if fam != 'cluster':  # the second vector only where the projector is measured
                v = v[:, :1]
            out['v'] = v
        w, V = np.linalg.eigh(x['a'])
        out['lapack'] = np.array(sc.heev_metrics(x['a'], w, V, out['w'], v))
    elif solver == 'solve':
        out['x'], out['info'] = mp_solve(x['a'], x['b'])
        out['lapack'] = np.array([sc.rel_fro(np.linalg.solve(x['a'], x['b']), out['x'])])
    elif solver == 'gev':
        out['w'], lam, out['info'] = mp_gev(x['t'], x['n'])
        out['lam'] = np.array(lam)
        _, V = scipy.linalg.eigh(x['t'], x['n'])
        out['lapack'] = np.array(sc.gev_metrics(x['t'], x['n'], V[:, -1], out['w'], lam)[:3])
        le, Ve = scipy.linalg.eig(x['t'], x['n'])
        k = int(np.argmax(le))
        ve = Ve[:, k] / np.linalg.norm(Ve[:, k])
        m = sc.gev_metrics(x['t'], x['n'], ve, out['w'], lam, le[k])
        out['lapack_eig'] = np.array([m[0], m[1], m[3]])
        if D <= sc.BEAMFORMER_MAX_D:
            ref = mp_beamformers(x['t'], x['n'], x['atf'], x['atf2'], out['w'], D)
            f64 = sc.beamformers_f64(x['t'], x['n'], x['atf'], x['atf2'], out['w'])
            out['bf_lapack'] = np.array([sc.rel_fro(f64[f], ref[f]) if f in ref else np.nan
                                         for f in sc.BEAMFORMER_FIELDS])
            if 'rule' in cases[key]:  # mat = G / tr G does not see the scaling: shared with the base
                del ref['souden_mat']
            if D > sc.BEAMFORMER_FULL_D:  # wmwf_mat = souden_mat * wmwf_scale (solver_cases.ref)
                del ref['wmwf_mat']
            else:
                del ref['wmwf_scale']
            out.update(ref)
    elif solver == 'gevgen':
        out['w'], lam, out['info'] = mp_gev_general(x['t'], x['n'])
        out['lam'] = np.array(lam)
        le, Ve = scipy.linalg.eig(x['t'], x['n'])
        k = int(np.argmax(le))
        m = sc.gev_metrics(x['t'], x['n'], Ve[:, k], out['w'], lam, le[k])
        out['lapack_eig'] = np.array([m[0], m[1], m[3]])
    reference.cache[key] = out
    return out


reference.cache = {}


def all_keys(cases):
    return list(cases) + [f'gevgen|nonherm|{D}' for D in sc.SIZES if D <= sc.PENCIL_MAX_D]


def build(verbose=False):
    cases = sc.build_cases()
    arrays = {}
    for key in all_keys(cases):
        for f, v in cases.get(key, {}).items():
            arrays[f'{key}|{f}'] = v
        for f, v in reference(cases, key).items():
            arrays[f'{key}|{f}'] = v
        if verbose:
            print(key, flush=True)
    return arrays


def serialise(arrays):
    """An .npz with fixed member order and time stamps, so that the same arrays give the same
    bytes (numpy.savez stamps the members with the current time)."""
    arrays = sc.pack_fixture(arrays)
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(arrays[name]), allow_pickle=False)
            z.writestr(info, member.getvalue())
    return buf.getvalue()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--check', action='store_true', help='compare with the committed fixture')
    ap.add_argument('--verbose', action='store_true')
    args = ap.parse_args(argv)
    blob = serialise(build(args.verbose))
    if args.check:
        with open(PATH, 'rb') as f:
            same = f.read() == blob
        print('identical' if same else 'DIFFERENT')
        return 0 if same else 1
    with open(PATH, 'wb') as f:
        f.write(blob)
    print(f'{PATH}: {len(blob)} bytes')
    return 0


if __name__ == '__main__':
    sys.exit(main())
