"""Inputs on which small dense solvers go wrong: the case list behind
tests/golden/solver_hard_cases.npz (recipe: oracle/make_solver_golden.py).

Pure NumPy and seeded: every call of `build_cases()` returns the same float64 arrays.  A case is
a dict of arrays keyed 'solver|family|D'.  To keep the fixture small, Hermitian inputs are stored
as their packed lower triangle, and the families that are an exact float64 function of another
stored matrix (a power-of-two multiple, its real part, its diagonal overwritten, ...) are stored
as that rule only: `expand()` rebuilds them bit for bit.  The error metrics that the recipe
records for LAPACK and that the tests apply to the device live here too, so that both sides
measure the same thing; nothing in this module needs more than NumPy.

Families (heev), each U diag(lambda) U^H with a random unitary U unless said otherwise:
  graded_k1e4 .. graded_k1e16   lambda log-spaced over the condition number
  cluster        lambda = 1, 1 - 1e-9, the rest log-spaced down to 1e-3
  indefinite     lambda evenly spaced on [-1, 1] (0 included for odd D)
  rank1, rankDm1 exact X X^H with 1 and D - 1 columns
  neardiag       diag(1..D) + 1e-10 (E + E^H), E = strict lower triangle of graded_k1e8
  eqdiag         graded_k1e8 with its diagonal overwritten by 0.5 (rotation branch d = 0)
  realsym        real part of graded_k1e8 (phase u = +-1)
  imagoff        diagonal of graded_k1e8, off-diagonal 1j * imag (phase u = +-i)
  scaled_p80, scaled_m80, scaled_p250, scaled_m250   graded_k1e8 times 2^+-80, 2^+-250
At D >= 17 one matrix per family: graded_k1e8 of the graded ones, rank1 of the rank-r ones.

solve: general U diag(sigma) V^H with kappa = 1e2 (M = D right-hand sides), 1e8 (M = 2), 1e12
(M = 1), plus kappa = 1e8 times 2^+-80; at D >= 17 the kappa = 1e8 systems only, and their matrix
is heev|graded_k1e8 with its rows rotated by one (P H = (P Q) diag(lambda) Q^H: the same singular
values, no symmetry left), which costs the fixture nothing.

gev (and gev_general, mvdr, mvdr_souden, wmwf, ban; lcmv up to D = 8, its limit): target =
a a^H + 1e-3 (graded kappa 1e2), noise graded with kappa = 1e2, 1e6, 1e10, an ATF a and a
second one for LCMV, plus the kappa = 1e6 pencil with target * 2^40 and noise * 2^-40; at D >= 17 the kappa = 1e6 pencils only.
gev_general additionally gets the non-Hermitian pencil (target: the solve|k1e8 matrix, at
D >= 17 heev|cluster with its rows rotated by one; noise: heev|graded_k1e8).
"""
import zlib

import numpy as np

SMALL = tuple(range(2, 10))          # every D in 2..8 and the first generic size
LARGE = (17, 32, 34)
SIZES = SMALL + LARGE
PENCIL_MAX_D = 32                    # gev, gev_general and solve stop here; heev goes to 34
BEAMFORMER_MAX_D = 32                # mvdr / souden / wmwf / ban references on every gev pencil
BEAMFORMER_FULL_D = 9                # up to here wmwf_mat is stored; above, as wmwf_scale (see ref)
LCMV_MAX_D = 8                       # pbbss_lcmv's limit

HEEV_STORED = ('graded_k1e4', 'graded_k1e8', 'graded_k1e12', 'graded_k1e16', 'cluster',
               'indefinite', 'rank1', 'rankDm1')
HEEV_STORED_LARGE = ('graded_k1e8', 'cluster', 'indefinite', 'rank1')
HEEV_DERIVED = {'neardiag': 'neardiag', 'eqdiag': 'eqdiag', 'realsym': 'real',
                'imagoff': 'imagoff', 'scaled_p80': 'scale:80', 'scaled_m80': 'scale:-80',
                'scaled_p250': 'scale:250', 'scaled_m250': 'scale:-250'}
HEEV_BASE = 'graded_k1e8'
SOLVE_STORED = {'k1e2': (1e2, 'D'), 'k1e8': (1e8, 2), 'k1e12': (1e12, 1)}
SOLVE_DERIVED = {'scaled_p80': 'scale:80', 'scaled_m80': 'scale:-80'}
SOLVE_BASE = 'k1e8'
GEV_STORED = {'noise_k1e2': 1e2, 'noise_k1e6': 1e6, 'noise_k1e10': 1e10}
GEV_BASE = 'noise_k1e6'
GEV_SCALED = 'scaled_40'             # target * 2^40, noise * 2^-40


def heev_families(D):
    stored = HEEV_STORED if D < 17 else HEEV_STORED_LARGE
    return tuple(stored) + tuple(HEEV_DERIVED)


def solve_families(D):
    stored = tuple(SOLVE_STORED) if D < 17 else (SOLVE_BASE,)
    return stored + tuple(SOLVE_DERIVED)


def gev_families(D):
    stored = tuple(GEV_STORED) if D < 17 else (GEV_BASE,)
    return stored + (GEV_SCALED,)


# ---------------------------------------------------------------- packing and derivation
def pack_lower(a):
    return np.ascontiguousarray(a[np.tril_indices(a.shape[0])])


def unpack_lower(p, D):
    a = np.zeros((D, D), dtype=np.complex128)
    a[np.tril_indices(D)] = p
    d = np.diag(a).real.copy()
    a = a + a.conj().T
    a[np.diag_indices(D)] = d
    return a


def expand(base, rule):
    """The derived input: an exact float64 function of the stored matrix `base`."""
    D = base.shape[0]
    off = ~np.eye(D, dtype=bool)
    if rule.startswith('scale:'):
        return np.ldexp(base.real, int(rule[6:])) + 1j * np.ldexp(base.imag, int(rule[6:]))
    if rule == 'roll':
        return np.ascontiguousarray(np.roll(base, 1, axis=0))
    if rule == 'real':
        return (base.real + 0j).astype(np.complex128)
    if rule == 'imagoff':
        return np.where(off, 1j * base.imag, base.real).astype(np.complex128)
    if rule == 'eqdiag':
        return np.where(off, base, 0.5).astype(np.complex128)
    if rule == 'neardiag':
        return np.where(off, 1e-10 * base, np.diag(np.arange(1.0, D + 1))).astype(np.complex128)
    raise ValueError(rule)


# ---------------------------------------------------------------- generators
def _rng(*key):
    return np.random.default_rng(zlib.crc32('|'.join(map(str, key)).encode()))


def _unitary(rng, D):
    z = rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D))
    q, r = np.linalg.qr(z)
    return q * (np.diag(r) / np.abs(np.diag(r)))


def _vector(rng, D):
    return rng.standard_normal(D) + 1j * rng.standard_normal(D)


def _hermitian(rng, lam):
    D = len(lam)
    u = _unitary(rng, D)
    return unpack_lower(pack_lower((u * lam) @ u.conj().T), D)


def _graded(D, kappa):
    return np.logspace(0.0, -np.log10(kappa), D)


def heev_spectrum(family, D):
    if family.startswith('graded_k'):
        return _graded(D, float(family[len('graded_k'):]))
    if family == 'cluster':
        return np.concatenate([[1.0, 1.0 - 1e-9], np.logspace(-1.0, -3.0, D - 2)])
    if family == 'indefinite':
        return np.linspace(-1.0, 1.0, D)
    raise ValueError(family)


def heev_stored(family, D):
    rng = _rng('heev', family, D)
    if family in ('rank1', 'rankDm1'):
        r = 1 if family == 'rank1' else D - 1
        x = rng.standard_normal((D, r)) + 1j * rng.standard_normal((D, r))
        return unpack_lower(pack_lower(x @ x.conj().T), D)
    return _hermitian(rng, heev_spectrum(family, D))


def solve_stored(family, D):
    kappa, M = SOLVE_STORED[family]
    M = D if M == 'D' else M
    rng = _rng('solve', family, D)
    u, v = _unitary(rng, D), _unitary(rng, D)
    a = (u * _graded(D, kappa)) @ v.conj().T
    b = rng.standard_normal((D, M)) + 1j * rng.standard_normal((D, M))
    return np.ascontiguousarray(a), b


def gev_stored(family, D):
    rng = _rng('gev', family, D)
    atf, atf2 = _vector(rng, D), _vector(rng, D)
    target = np.outer(atf, atf.conj()) + 1e-3 * _hermitian(rng, _graded(D, 1e2))
    target = unpack_lower(pack_lower(target), D)
    noise = _hermitian(rng, _graded(D, GEV_STORED[family]))
    return target, noise, atf, atf2


def build_cases():
    """{'solver|family|D': {field: array}}: the inputs exactly as the fixture stores them
    (stored families: packed arrays; derived families: the rule as a string)."""
    cases = {}
    for D in SIZES:
        for fam in heev_families(D):
            key = f'heev|{fam}|{D}'
            if fam in HEEV_DERIVED:
                cases[key] = {'rule': np.array(HEEV_DERIVED[fam])}
            else:
                cases[key] = {'a': pack_lower(heev_stored(fam, D))}
        for fam in solve_families(D) if D <= PENCIL_MAX_D else ():
            key = f'solve|{fam}|{D}'
            if fam in SOLVE_DERIVED:
                cases[key] = {'rule': np.array(SOLVE_DERIVED[fam])}
            elif D >= 17:
                cases[key] = {'rule': np.array('roll'), 'b': solve_stored(fam, D)[1]}
            else:
                a, b = solve_stored(fam, D)
                cases[key] = {'a': a, 'b': b}
        for fam in gev_families(D) if D <= PENCIL_MAX_D else ():
            key = f'gev|{fam}|{D}'
            if fam == GEV_SCALED:
                cases[key] = {'rule': np.array('scale:40')}
            else:
                t, n, atf, atf2 = gev_stored(fam, D)
                cases[key] = {'t': pack_lower(t), 'n': pack_lower(n), 'atf': atf, 'atf2': atf2}
    return cases


def inputs(cases, key):
    """Full float64 inputs of case `key` (derived ones rebuilt from their base)."""
    solver, fam, D = key.split('|')
    D = int(D)
    c = cases.get(key)
    if solver == 'heev':
        if 'rule' in c:
            base = unpack_lower(cases[f'heev|{HEEV_BASE}|{D}']['a'], D)
            return {'a': expand(base, str(c['rule']))}
        return {'a': unpack_lower(c['a'], D)}
    if solver == 'solve':
        if 'rule' in c and str(c['rule']) == 'roll':
            return {'a': expand(inputs(cases, f'heev|{HEEV_BASE}|{D}')['a'], 'roll'), 'b': c['b']}
        if 'rule' in c:
            base = inputs(cases, f'solve|{SOLVE_BASE}|{D}')
            return {'a': expand(base['a'], str(c['rule'])), 'b': base['b']}
        return {'a': c['a'], 'b': c['b']}
    if solver == 'gev':
        if 'rule' in c:
            base = cases[f'gev|{GEV_BASE}|{D}']
            s = int(str(c['rule'])[6:])
            return {'t': expand(unpack_lower(base['t'], D), f'scale:{s}'),
                    'n': expand(unpack_lower(base['n'], D), f'scale:{-s}'),
                    'atf': base['atf'], 'atf2': base['atf2']}
        return {'t': unpack_lower(c['t'], D), 'n': unpack_lower(c['n'], D), 'atf': c['atf'],
                'atf2': c['atf2']}
    if solver == 'gevgen':  # the non-Hermitian pencil borrows its matrices
        t = (cases[f'solve|{SOLVE_BASE}|{D}']['a'] if D < 17 else
             expand(inputs(cases, f'heev|cluster|{D}')['a'], 'roll'))
        return {'t': t, 'n': inputs(cases, f'heev|{HEEV_BASE}|{D}')['a']}
    raise ValueError(key)


# ---------------------------------------------------------------- metrics
# Everything below is evaluated in extended precision (np.longdouble) from float64 arrays, so the
# rounding of the measurement stays well under the float64 errors that it measures.
EPS = float(np.finfo(np.float64).eps)
_LD = np.clongdouble


def _unit(v):
    v = np.asarray(v, dtype=_LD)
    return v / np.sqrt(np.sum(np.abs(v) ** 2))


def sin_angle(v, ref):
    """sin of the angle between the lines spanned by v and ref."""
    v, r = _unit(v), _unit(ref)
    return float(np.sqrt(np.sum(np.abs(v - r * np.vdot(r, v)) ** 2)))


def rel_fro(x, ref):
    x, ref = np.asarray(x, dtype=_LD), np.asarray(ref, dtype=_LD)
    return float(np.sqrt(np.sum(np.abs(x - ref) ** 2)) / np.sqrt(np.sum(np.abs(ref) ** 2)))


def _projector2(v1, v2):
    r1 = _unit(v1)
    r2 = np.asarray(v2, dtype=_LD)
    r2 = _unit(r2 - r1 * np.vdot(r1, r2))
    return np.outer(r1, r1.conj()) + np.outer(r2, r2.conj())


def heev_metrics(a, w, V, ref_w, ref_v):
    """(eigenvalue error, residual ||A V - V L||_F, orthogonality defect, sin of the principal
    angle, error of the projector on the two leading vectors) of an eigendecomposition (w
    ascending, V[:, k] belongs to w[k]) against the reference eigenvalues ref_w and the two
    leading reference eigenvectors ref_v[:, 0] (principal) and ref_v[:, 1]."""
    D = a.shape[0]
    al, Vl, wl = a.astype(_LD), np.asarray(V, dtype=_LD), np.asarray(w, dtype=np.longdouble)
    val = float(np.max(np.abs(wl - np.asarray(ref_w, dtype=np.longdouble))))
    res = float(np.sqrt(np.sum(np.abs(al @ Vl - Vl * wl) ** 2)))
    orth = float(np.max(np.abs(Vl.conj().T @ Vl - np.eye(D))))
    ang = sin_angle(V[:, -1], ref_v[:, 0])
    proj = np.nan  # only where the second reference vector is kept (the cluster family)
    if ref_v.shape[1] > 1:
        dp = _projector2(V[:, -1], V[:, -2]) - _projector2(ref_v[:, 0], ref_v[:, 1])
        proj = float(np.linalg.norm(dp.astype(np.complex128), 2))
    return val, res, orth, ang, proj


def gev_metrics(t, n, w, ref_w, ref_lam, lam=None):
    """(relative error of the Rayleigh quotient w^H T w / w^H N w, sin of the angle to the
    reference vector, |w^H N w - 1|, relative error of a returned eigenvalue or 0)."""
    wl = np.asarray(w, dtype=_LD)
    wtw = np.vdot(wl, t.astype(_LD) @ wl)
    wnw = np.vdot(wl, n.astype(_LD) @ wl)
    rq = float(abs(wtw / wnw - _LD(ref_lam)) / abs(ref_lam))
    ret = 0.0 if lam is None else float(abs(_LD(lam) - _LD(ref_lam)) / abs(ref_lam))
    return rq, sin_angle(w, ref_w), float(abs(wnw - 1)), ret


def beamformers_f64(t, n, atf, atf2, w):
    """The formulas of oracle/beamformer.py in plain float64 NumPy on one pencil: what LAPACK's
    solve gives.  Keys as the reference arrays of the fixture."""
    tiny = np.finfo(np.float64).tiny
    g = np.linalg.solve(n, t)
    tr = np.trace(g)
    mat = g / max(tr.real, tiny)
    out = {'souden_mat': mat,
           'souden_num': np.einsum('dr,de,er->r', mat.conj(), t, mat),
           'souden_den': np.einsum('dr,de,er->r', mat.conj(), n, mat),
           'wmwf_mat': g / (1.0 + tr)}
    x = np.linalg.solve(0.5 * (n + n.conj().T), atf)
    out['mvdr'] = x / np.vdot(atf, x)
    nom = np.sqrt(np.vdot(w, n @ (n @ w)))
    den = np.vdot(w, n @ w)
    out['ban'] = w * abs(nom / abs(den))
    if len(atf) <= LCMV_MAX_D:
        h = np.stack([atf, atf2])                  # (K, D)
        pih = np.linalg.solve(n, h.T)              # (D, K): column k = N^-1 a_k
        temp = np.linalg.solve(h.conj() @ pih, LCMV_RESPONSE.astype(np.complex128))
        out['lcmv'] = pih @ temp
    return out


LCMV_RESPONSE = np.array([1.0, 0.5])
BEAMFORMER_FIELDS = ('mvdr', 'souden_mat', 'souden_num', 'souden_den', 'wmwf_mat', 'ban', 'lcmv')


# ---------------------------------------------------------------- the fixture file
# One complex and one float64 blob plus a JSON index: a zip member per array would cost more bytes
# in headers than the arrays hold.
def pack_fixture(arrays):
    import json
    index, blobs = {}, {'c': [], 'f': []}
    offs = {'c': 0, 'f': 0}
    for name in sorted(arrays):
        v = np.asarray(arrays[name])
        if v.dtype.kind == 'U':
            index[name] = str(v)
            continue
        kind = 'c' if v.dtype.kind == 'c' else 'f'
        flat = v.astype(np.complex128 if kind == 'c' else np.float64).ravel()
        index[name] = [kind, offs[kind], list(v.shape)]
        blobs[kind].append(flat)
        offs[kind] += flat.size
    return {'index': np.frombuffer(json.dumps(index, sort_keys=True).encode(), dtype=np.uint8),
            'c128': np.concatenate(blobs['c']), 'f64': np.concatenate(blobs['f'])}


def load_fixture(path):
    """-> {'solver|family|D|field': array or rule string}"""
    import json
    with np.load(path) as z:
        index = json.loads(bytes(z['index']).decode())
        blobs = {'c': z['c128'], 'f': z['f64']}
    out = {}
    for name, e in index.items():
        if isinstance(e, str):
            out[name] = e
        else:
            n = int(np.prod(e[2], dtype=np.int64))
            out[name] = blobs[e[0]][e[1]:e[1] + n].reshape(e[2])
    return out


def fixture_cases(fx):
    """The `cases` dict of build_cases() back from a loaded fixture (input fields only)."""
    cases = {}
    for name, v in fx.items():
        key, field = name.rsplit('|', 1)
        if field in ('a', 'b', 't', 'n', 'atf', 'atf2', 'rule'):
            cases.setdefault(key, {})[field] = v
    return cases


def ref(fx, key, field):
    """Reference array of a case; a derived case without it shares the one of its base."""
    if f'{key}|{field}' in fx:
        return fx[f'{key}|{field}']
    if field == 'wmwf_mat' and f'{key}|wmwf_scale' in fx:
        # G / (1 + tr G) = [G / Re tr G] * [Re tr G / (1 + tr G)]: at D >= 17 the fixture keeps the
        # second factor (one number, rounded from 50 digits) in place of a second D x D matrix.
        # The product of two correctly rounded factors is within 3 eps of the exact entry, against
        # a floor of D eps kappa(N) >= 1e7 eps for these cases.
        return ref(fx, key, 'souden_mat') * fx[f'{key}|wmwf_scale']
    solver, _, D = key.split('|')
    base = {'heev': HEEV_BASE, 'solve': SOLVE_BASE, 'gev': GEV_BASE}[solver]
    return fx[f'{solver}|{base}|{D}|{field}']


# ---------------------------------------------------------------- first-order error bounds
# The textbook forward errors of a backward stable solver, in the order of the metric tuples
# above; `info` is the case's array of that name (all of it measured in multiprecision).
def heev_floors(D, info):
    norm2, _, relgap, relgap_pair = (float(x) for x in info)
    return (D * EPS * norm2, D * EPS * norm2, D * EPS, D * EPS / relgap, D * EPS / relgap_pair)


def solve_floor(D, info):
    return D * EPS * float(info[1])


def gev_floors(D, info):
    kappa, relgap = float(info[0]), float(info[1])
    return (D * EPS * kappa, D * EPS * kappa / relgap, D * EPS * kappa, D * EPS * kappa)
