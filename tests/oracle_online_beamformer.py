"""NumPy restatement of the frame-recursive mask-driven MVDR beamformer: the yardstick of
pb_bss_amd.extraction.recursive_mvdr_souden and OnlineMVDR.

Written from the definition in the module docstring of
pb_bss_amd/extraction/online_beamformer.py.  No package implements that definition under this
name, so there is nothing else to compare with.  What is checked
(tests/test_online_beamformer_oracle.py) is the restatement against the same recursion in
numpy.clongdouble, whose distance from the float64 run is the restatement's own error `e_case`,
and against a route that shares nothing with the recursion: after T frames the statistics are
plain exponentially weighted sums and the last vector is the batch Souden solution of them.

One problem is Y (D, T) with masks (T,); `recursive` takes (..., D, T) / (..., T) and loops over
the leading axes.
"""
import numpy as np

TINY = np.finfo(np.float64).tiny


def _mirror(P):
    """The lower triangle, a real diagonal, the upper triangle its conjugate mirror."""
    low = np.tril(P, -1)
    return low + low.conj().T + np.diag(np.diag(P).real)


def _one(Y, s, v, alpha, ref, p0, ctype, state=None):
    """-> (X (T,), W (T, D), Phi (D, D), Psi (D, D), flagged) in the precision of ctype."""
    rtype = np.zeros(1, ctype).real.dtype.type
    D, T = Y.shape
    Y = Y.astype(ctype)
    s, v = np.asarray(s).astype(rtype), np.asarray(v).astype(rtype)
    alpha = rtype(alpha)
    if state is None:
        Phi = np.zeros((D, D), ctype)
        Psi = (np.eye(D) / rtype(p0)).astype(ctype)
    else:
        Phi, Psi = (np.array(a, ctype) for a in state)
    X = np.empty(T, ctype)
    W = np.empty((T, D), ctype)
    dead = False
    with np.errstate(all='ignore'):
        for t in range(T):
            if dead:
                X[t], W[t] = np.nan, np.nan
                continue
            y = Y[:, t]
            Phi = _mirror(alpha * Phi + s[t] * np.outer(y, y.conj()))
            n = Psi @ y
            den = alpha + v[t] * np.sum(y.real * n.real + y.imag * n.imag)
            if not (den > 0 and np.isfinite(den)):
                dead = True   # from this frame on
                X[t], W[t] = np.nan, np.nan
                continue
            Psi = _mirror((Psi - np.outer((v[t] / den) * n, n.conj())) / alpha)
            u = Phi[:, ref]
            lam = np.sum(Psi.real * Phi.real + Psi.imag * Phi.imag)
            w = (Psi @ u) / max(lam, rtype(TINY))
            x = np.sum(w.conj() * y)
            if not (np.isfinite(lam) and np.isfinite(x)):
                dead = True
                X[t], W[t] = np.nan, np.nan
                continue
            X[t], W[t] = x, w
    if dead:
        Phi, Psi = np.full_like(Phi, np.nan), np.full_like(Psi, np.nan)
    return X, W, Phi, Psi, dead


def recursive(Y, target_mask, noise_mask, alpha, ref, p0, ctype=np.complex128, state=None):
    """(..., D, T), (..., T), (..., T) -> (X (..., T), W (T, ..., D), target_psd (..., D, D),
    noise_inv (..., D, D), flagged (...)) from Phi = 0, Psi = I / p0, or from
    state = (target_psd, noise_inv)."""
    Y = np.asarray(Y)
    lead = Y.shape[:-2]
    flat = Y.reshape((-1,) + Y.shape[-2:])
    s = np.asarray(target_mask).reshape(len(flat), -1)
    v = np.asarray(noise_mask).reshape(len(flat), -1)
    st = None if state is None else [np.asarray(a).reshape((-1,) + a.shape[-2:]) for a in state]
    outs = [_one(y, s[i], v[i], alpha, ref, p0, ctype,
                 None if st is None else (st[0][i], st[1][i])) for i, y in enumerate(flat)]
    X, W, Phi, Psi, flag = (np.stack([o[i] for o in outs]) for i in range(5))
    D, T = Y.shape[-2:]
    return (X.reshape(lead + (T,)), np.moveaxis(W, 1, 0).reshape((T,) + lead + (D,)),
            Phi.reshape(lead + (D, D)), Psi.reshape(lead + (D, D)), flag.reshape(lead))


def batch_statistics(Y, s, v, alpha, p0):
    """(D, T), (T,), (T,) -> (Phi, Psi^-1) after T frames as plain weighted sums."""
    D, T = Y.shape
    Y = Y.astype(np.complex128)
    g = alpha ** np.arange(T - 1, -1, -1.0)
    Phi = np.einsum('t,dt,et->de', g * s, Y, Y.conj())
    N = alpha ** T * p0 * np.eye(D) + np.einsum('t,dt,et->de', g * v, Y, Y.conj())
    return Phi, N


def batch_souden(Phi, N, ref):
    """The Souden MVDR vector N^-1 Phi[:, ref] / tr(N^-1 Phi) by numpy.linalg.solve, and cond(N)."""
    A = np.linalg.solve(N, Phi)
    return A[:, ref] / max(np.trace(A).real, TINY), np.linalg.cond(N)


# ---- the sweep of tests/test_gpu_online_beamformer.py: (D, T) ------------------------------------
BATCH = 3
TILE = 32   # the kernel's frame tile (pb_bss_amd.engine.ONLINE_BF_TILE)
TABLE_CASES = [(1, 8), (2, 64), (3, 65), (4, 130), (5, 33), (8, 300), (16, 200), (2, 1000)]
# what the kernel's plan adds: T one below, at and one above the frame tile (twice the tile is
# (2, 64) of the table); D = 9 and D = 12: the middle of the 16-sensor instantiation
PLAN_CASES = [(2, TILE - 1), (2, TILE), (2, TILE + 1), (9, 70), (12, 70)]
CASES = TABLE_CASES + PLAN_CASES
ALPHAS = (1.0, 0.999, 0.95)
P0 = 0.1


def ref_channel(case):
    """D - 1, so that an indexing slip on the reference channel shows."""
    return case[0] - 1


def case_input(case, dtype=np.complex128):
    """-> (Y (BATCH, D, T) of dtype, target_mask (BATCH, T), noise_mask (BATCH, T) float64).

    A rank-one target active in about 60 % of the frames plus sensor noise of standard deviation
    0.3.  Target mask: a clipped noisy ratio mask, exactly zero in every 7th frame from frame 0
    (so Phi = 0 and w = 0 at the first frame); noise mask: one minus the target mask, exactly zero
    in every 11th frame from frame 3."""
    D, T = case
    rng = np.random.default_rng(1000 * D + T)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    steer = cn(BATCH, D, 1)
    active = rng.uniform(size=(BATCH, T)) < 0.6
    target = steer * (cn(BATCH, 1, T) * active[:, None, :])
    noise = 0.3 * cn(BATCH, D, T)
    Y = target + noise
    pt = np.mean(np.abs(target) ** 2, axis=1)
    pn = np.mean(np.abs(noise) ** 2, axis=1)
    s = np.clip(pt / (pt + pn) + 0.1 * rng.standard_normal((BATCH, T)), 0.0, 1.0)
    s[:, 0::7] = 0.0
    v = 1.0 - s
    v[:, 3::11] = 0.0
    return Y.astype(dtype), s, v


def measure_e_case(case, alpha, dtype=np.complex128):
    """(eX, eW, ePhi, ePsi): the float64 restatement against the longdouble one, each relative to
    the maximum magnitude of the quantity."""
    Y, s, v = case_input(case, dtype)
    a = recursive(Y, s, v, alpha, ref_channel(case), P0)
    b = recursive(Y, s, v, alpha, ref_channel(case), P0, ctype=np.clongdouble)
    assert not a[4].any() and not b[4].any()
    return tuple(float(np.max(np.abs(a[i] - b[i])) / np.max(np.abs(b[i]))) for i in range(4))
