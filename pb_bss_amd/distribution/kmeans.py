"""k-means on real embeddings on the device, and the two classes of the reference that stand on
it: `BinaryGMM` and `BinaryGMMTrainer` (pb_bss/distribution/gmm.py:176-230, which hand the work to
sklearn.cluster.KMeans).

`KMeans` is the subset of sklearn's estimator the reference uses, on the kernels of
csrc/kmeans.hip: one C-ABI call per run (`pbbss_kmeans_fit`: Lloyd sweeps with sklearn's stopping
rule and empty-cluster relocation, the stop taken on the device), one per seeding
(`pbbss_kmeans_plusplus`: greedy k-means++ on random numbers the host draws in sklearn's order
from a numpy RandomState) and one per prediction (`pbbss_kmeans_predict`).

The arithmetic is float64 on the exactly widened values, with the squared distance taken as the
direct sum of (x_e - c_e)^2.  For float32 input the results are therefore those of sklearn on
x.astype(float64), not those of its float32 arithmetic.

NumPy in gives NumPy out.  A device tensor in gives device tensors out, and the only host
synchronisation then is the stop flag, read once per block of iterations.
"""
from dataclasses import dataclass

import numpy as np

from .. import _lib
from .utils import _ProbabilisticModel, as_result

__all__ = ['KMeans', 'BinaryGMM', 'BinaryGMMTrainer']

MAX_CLASSES = 64     # csrc/kmeans.hpp: kKmeansMaxK
MAX_FEATURES = 256   # kKmeansMaxE
DEFAULT_BLOCK = 8    # Lloyd iterations enqueued between two reads of the stop flag


def _check_random_state(seed):
    """None: numpy's global RandomState; an int: a fresh one; a RandomState: itself
    (sklearn.utils.check_random_state)."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f'{seed!r} cannot be used to seed a numpy.random.RandomState instance')


def _default_trials(n_clusters):
    return 2 + int(np.log(n_clusters))


def draw_randoms(random_state, n_clusters, trials):
    """The numbers greedy k-means++ takes from a RandomState, in sklearn's order: the uniform
    behind choice(n, p=uniform), then uniform(size=trials) for each further centre."""
    out = [random_state.random_sample()]
    for _ in range(n_clusters - 1):
        out.extend(random_state.uniform(size=trials))
    return np.asarray(out, np.float64)


def _rows(x):
    """x (..., N, E) real -> (device tensor (B, N, E) float32 / float64, leading shape)."""
    t = _lib.require_gpu()
    if _lib.is_torch(x):
        assert not x.is_complex(), x.dtype
    else:
        x = np.asarray(x)
        assert np.isrealobj(x), x.dtype
    if x.ndim < 2:
        raise ValueError(f'expected (..., N, E), got shape {tuple(x.shape)}')
    xd = _lib.to_device(x)
    if xd.dtype not in (t.float32, t.float64):
        xd = xd.to(t.float64)
    lead = tuple(xd.shape[:-2])
    N, E = xd.shape[-2:]
    if N < 1 or E < 1 or int(np.prod(lead, dtype=np.int64)) < 1:
        raise ValueError(f'empty input: shape {tuple(xd.shape)}')
    if E > MAX_FEATURES:
        raise NotImplementedError(f'k-means serves up to {MAX_FEATURES} features, got {E}')
    return xd.reshape(-1, N, E).contiguous(), lead


def _saliency_rows(saliency, lead, N, device):
    """saliency (N,) or (..., N) bool -> (device uint8 (B, N), selected rows per problem when they
    are known without a device round trip)."""
    if saliency is None:
        return None, None
    t = _lib.torch()
    on_device = _lib.is_torch(saliency)
    if on_device:
        assert saliency.dtype == t.bool, (
            f'Only boolean saliency supported. Current dtype: {saliency.dtype}.')
        sal = saliency.to(device)
        count = None
    else:
        saliency = np.asarray(saliency)
        assert saliency.dtype == bool, (
            f'Only boolean saliency supported. Current dtype: {saliency.dtype}.')
        full = np.broadcast_to(saliency, lead + (N,))
        count = int(full.reshape(-1, N).sum(axis=1).min())
        sal = t.from_numpy(np.array(full)).to(device)  # a copy: the broadcast view is read-only
    sal = sal.expand(lead + (N,)).reshape(-1, N).to(t.uint8).contiguous()
    return sal, count


def _too_few(n_samples, n_clusters):
    return ValueError(f'n_samples={n_samples} should be >= n_clusters={n_clusters}.')


def _call_fit(xd, K, sal, centers, max_iter, tol, block):
    t = _lib.torch()
    B, N, E = xd.shape
    out_c = t.empty((B, K, E), dtype=t.float64, device=xd.device)
    labels = t.empty((B, N), dtype=t.int32, device=xd.device)
    inertia = t.empty((B,), dtype=t.float64, device=xd.device)
    n_iter = t.empty((B,), dtype=t.int32, device=xd.device)
    rc = _lib.launch('pbbss_kmeans_fit', xd.device, xd, xd.dtype == t.float64, B, N, E, K, sal,
                     centers, max_iter, tol, block, out_c, labels, inertia, n_iter,
                     what=f'kmeans_fit(B={B}, N={N}, E={E}, K={K})',
                     accept=() if sal is None else (_lib.ERR_INVALID_ARG,))
    if rc == _lib.ERR_INVALID_ARG:
        # every other argument was validated here: a problem selects fewer rows than classes
        raise _too_few('(selected rows)', K)
    return out_c, labels, inertia, n_iter


def _call_predict(xd, centers, one_hot=False, inertia=False):
    t = _lib.torch()
    B, N, E = xd.shape
    K = centers.shape[1]
    labels = t.empty((B, N), dtype=t.int32, device=xd.device)
    hot = t.empty((B, K, N), dtype=xd.dtype, device=xd.device) if one_hot else None
    val = t.empty((B,), dtype=t.float64, device=xd.device) if inertia else None
    _lib.launch('pbbss_kmeans_predict', xd.device, xd, xd.dtype == t.float64, B, N, E, K, centers,
                labels, hot, val, what=f'kmeans_predict(B={B}, N={N}, E={E}, K={K})')
    return labels, hot, val


def _call_plusplus(xd, K, sal, randoms, trials):
    t = _lib.torch()
    B, N, E = xd.shape
    rnd = t.from_numpy(np.ascontiguousarray(randoms, np.float64)).to(xd.device)
    indices = t.empty((B, K), dtype=t.int32, device=xd.device)
    centers = t.empty((B, K, E), dtype=t.float64, device=xd.device)
    _lib.launch('pbbss_kmeans_plusplus', xd.device, xd, xd.dtype == t.float64, B, N, E, K, sal,
                trials, rnd, indices, centers,
                what=f'kmeans_plusplus(B={B}, N={N}, E={E}, K={K})')
    return indices, centers


def kmeans_plusplus(x, n_clusters, *, saliency=None, random_state=None, n_local_trials=None):
    """Greedy k-means++ seeding of x (..., N, E) -> (centers (..., K, E) in the dtype of x,
    indices (..., K) int32), as sklearn.cluster.kmeans_plusplus draws them from the same
    RandomState (up to 8 local trials)."""
    like_torch = _lib.is_torch(x)
    xd, lead = _rows(x)
    B, N, E = xd.shape
    K = int(n_clusters)
    sal, count = _saliency_rows(saliency, lead, N, xd.device)
    if not 1 <= K <= MAX_CLASSES:
        raise NotImplementedError(f'k-means serves 1 to {MAX_CLASSES} classes, got {K}')
    if K > (N if count is None else count):
        raise _too_few(N if count is None else count, K)
    trials = _default_trials(K) if n_local_trials is None else int(n_local_trials)
    rs = _check_random_state(random_state)
    randoms = np.stack([draw_randoms(rs, K, trials) for _ in range(B)])
    indices, centers = _call_plusplus(xd, K, sal, randoms, trials)
    return (as_result(centers.to(xd.dtype).reshape(lead + (K, E)), like_torch),
            as_result(indices.reshape(lead + (K,)), like_torch))


class KMeans:
    """The part of sklearn.cluster.KMeans the reference uses, on the device.

    init: 'k-means++' (greedy, sklearn's draws), 'random' (host-drawn choice(N, K,
    replace=False) among the selected rows) or an array (..., K, E).  n_init='auto' means 1 for
    'k-means++' and for an array, 10 for 'random'; the run with the lowest inertia wins, the
    first one among equals.  x may carry leading independent axes (..., N, E): all problems
    run in one launch and the attributes carry the leading axes.

    The arithmetic is float64 on the exactly widened values: for float32 input the results are
    those of sklearn on x.astype(float64), not those of its float32 arithmetic.
    """

    def __init__(self, n_clusters, init='k-means++', n_init='auto', max_iter=300, tol=1e-4,
                 random_state=None):
        self.n_clusters = n_clusters
        self.init = init
        self.n_init = n_init
        self.max_iter = max_iter
        self.tol = tol
        self.random_state = random_state

    def _runs(self):
        if self.n_init == 'auto':
            return 10 if isinstance(self.init, str) and self.init == 'random' else 1
        n = int(self.n_init)
        if n < 1:
            raise ValueError(f'n_init should be > 0, got {self.n_init}')
        return n if isinstance(self.init, str) else 1  # an array gives the same run every time

    def _initial_centers(self, xd, lead, sal, rs):
        t = _lib.torch()
        B, N, E = xd.shape
        K = self.n_clusters
        if isinstance(self.init, str):
            if self.init == 'k-means++':
                trials = _default_trials(K)
                randoms = np.stack([draw_randoms(rs, K, trials) for _ in range(B)])
                return _call_plusplus(xd, K, sal, randoms, trials)[1]
            if self.init == 'random':
                rows = None if sal is None else _lib.to_host(sal).astype(bool)
                idx = np.empty((B, K), np.int64)
                for b in range(B):
                    if rows is None:
                        idx[b] = rs.choice(N, K, replace=False)
                    else:
                        chosen = np.flatnonzero(rows[b])
                        if K > chosen.size:
                            raise _too_few(chosen.size, K)
                        idx[b] = chosen[rs.choice(chosen.size, K, replace=False)]
                idx = t.from_numpy(idx).to(xd.device)
                return xd[t.arange(B, device=xd.device)[:, None], idx].to(t.float64).contiguous()
            raise ValueError(f"init should be 'k-means++', 'random' or an array, got {self.init!r}")
        init = _lib.to_device(self.init, device=xd.device).to(t.float64)
        if tuple(init.shape[-2:]) != (K, E):
            raise ValueError(f'The shape of the initial centers {tuple(init.shape)} does not match '
                             f'(n_clusters, n_features) = {(K, E)}.')
        return init.expand(lead + (K, E)).reshape(B, K, E).contiguous()

    def fit(self, x, saliency=None, *, block=None):
        """x (..., N, E) real, saliency (N,) or (..., N) bool or None.  `block`: Lloyd iterations
        enqueued between two reads of the stop flag; the results do not depend on it."""
        K = int(self.n_clusters)
        like_torch = _lib.is_torch(x)
        xd, lead = _rows(x)
        t = _lib.torch()
        B, N, E = xd.shape
        if not 1 <= K <= MAX_CLASSES:
            raise NotImplementedError(f'k-means serves 1 to {MAX_CLASSES} classes, got {K}')
        if int(self.max_iter) < 1:
            raise ValueError(f'max_iter should be > 0, got {self.max_iter}')
        if not float(self.tol) >= 0:
            raise ValueError(f'tol should be >= 0, got {self.tol}')
        sal, count = _saliency_rows(saliency, lead, N, xd.device)
        if K > (N if count is None else count):
            raise _too_few(N if count is None else count, K)
        block = DEFAULT_BLOCK if block is None else int(block)
        if block < 1:
            raise ValueError(f'block should be > 0, got {block}')
        rs = _check_random_state(self.random_state)
        best = None
        for _ in range(self._runs()):
            init = self._initial_centers(xd, lead, sal, rs)
            run = _call_fit(xd, K, sal, init, self.max_iter, self.tol, block)
            if best is None:
                best = run
            else:  # per problem: the lower inertia, the earlier run among equals
                better = run[2] < best[2]
                best = tuple(t.where(better.reshape((B,) + (1,) * (new.dim() - 1)), new, old)
                             for new, old in zip(run, best))
        centers, labels, inertia, n_iter = best
        self.cluster_centers_ = as_result(centers.to(xd.dtype).reshape(lead + (K, E)), like_torch)
        self.labels_ = as_result(labels.reshape(lead + (N,)), like_torch)
        self.inertia_ = as_result(inertia.reshape(lead), like_torch)
        self.n_iter_ = as_result(n_iter.reshape(lead), like_torch)
        if not like_torch and not lead:
            self.inertia_ = float(self.inertia_)
            self.n_iter_ = int(self.n_iter_)
        self.n_features_in_ = E
        return self

    def predict(self, x):
        """x (..., N, E) -> labels (..., N) int32 of the nearest centre."""
        like_torch = _lib.is_torch(x)
        xd, lead = _rows(x)
        centers = _centers_for(self.cluster_centers_, xd, lead)
        labels, _, _ = _call_predict(xd, centers)
        return as_result(labels.reshape(lead + (xd.shape[1],)), like_torch)

    def fit_predict(self, x, saliency=None):
        return self.fit(x, saliency).labels_


def _centers_for(cluster_centers, xd, lead):
    """cluster_centers_ (K, E) or (..., K, E), NumPy or tensor, any real dtype ->
    device (B, K, E) float64."""
    t = _lib.torch()
    c = _lib.to_device(cluster_centers, device=xd.device).to(t.float64)
    E = xd.shape[-1]
    if c.dim() < 2 or c.shape[-1] != E:
        raise ValueError(f'cluster centres {tuple(c.shape)} do not match {E} features')
    K = c.shape[-2]
    if not 1 <= K <= MAX_CLASSES:
        raise NotImplementedError(f'k-means serves 1 to {MAX_CLASSES} classes, got {K}')
    return c.expand(lead + (K, E)).reshape(-1, K, E).contiguous()


@dataclass
class BinaryGMM(_ProbabilisticModel):
    """Hard-decision mixture: one-hot affiliations of a fitted k-means (gmm.py:176-198).
    `kmeans` is anything with `cluster_centers_` and `n_clusters` -- the `KMeans` of this module
    or a fitted sklearn.cluster.KMeans; the prediction runs on the device either way."""
    kmeans: object = None

    def predict(self, x):
        """x (N, D) real -> affiliation (K, N) in x.dtype; leading independent axes
        (..., N, D) -> (..., K, N)."""
        like_torch = _lib.is_torch(x)
        if not like_torch:
            x = np.asarray(x)
            assert np.isrealobj(x), x.dtype
        xd, lead = _rows(x)
        N = xd.shape[1]
        centers = _centers_for(self.kmeans.cluster_centers_, xd, lead)
        K = centers.shape[1]
        assert K == self.kmeans.n_clusters, (K, self.kmeans.n_clusters)
        _, hot, _ = _call_predict(xd, centers, one_hot=True)
        hot = hot.reshape(lead + (K, N))
        if like_torch:
            return hot if hot.dtype == x.dtype else hot.to(x.dtype)
        return _lib.to_host(hot).astype(x.dtype, copy=False)


class BinaryGMMTrainer:
    """k-means trainer for Deep Clustering embeddings (gmm.py:201-230), on the device."""

    def fit(self, x, num_classes, saliency=None, *, initialization=None, random_state=None):
        """x (N, D) real, num_classes > 0, saliency (N,) bool or None: rows with False take part
        in no statistic, so the result equals the fit on x[saliency].

        Beyond the reference: `initialization` (K, D) centres instead of the k-means++ seeding,
        `random_state` (None: numpy's global RandomState, as sklearn), and leading independent
        axes (..., N, D) fitted in one launch."""
        N = x.shape[-2]
        if saliency is not None:
            kind = saliency.dtype
            assert str(kind).endswith('bool'), (
                f'Only boolean saliency supported. Current dtype: {kind}.')
            assert tuple(saliency.shape) == (N,), (tuple(saliency.shape), N)
        init = 'k-means++' if initialization is None else initialization
        kmeans = KMeans(n_clusters=num_classes, init=init, random_state=random_state)
        return BinaryGMM(kmeans=kmeans.fit(x, saliency))
