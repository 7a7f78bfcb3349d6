"""Deterministic initialisations (reference: pb_bss/initializer/deterministic.py)."""
import numpy as np

from .. import _lib


def flag(
        Y,
        num_classes: int,
        permutation_free: bool = False,
        minimum: float = 0,
):
    """The time axis cut into `num_classes` consecutive segments, segment k given to class k.

    With 0 < minimum < 1 / num_classes no affiliation is exactly zero: the other classes get
    `minimum`, the segment's own class the rest.  Only the permutation-free form exists (the same
    (K, N) pattern for every independent axis).

    Args:
        Y: (..., N, D), NumPy array or device tensor; only its shape is used
    Returns:
        (..., K, N) of the kind of `Y`
    """
    if not permutation_free:
        raise NotImplementedError(permutation_free)
    K = int(num_classes)
    *independent, N, _ = tuple(Y.shape)
    owner = np.linspace(0, K, N, dtype=int, endpoint=False)
    pattern = (owner == np.arange(K)[:, None]).astype(np.float64)
    if minimum != 0:
        assert 0 < minimum < (1 / K), (minimum, K)
        pattern = np.maximum(pattern, minimum / (1 - (K - 1) * minimum))
        pattern = pattern / np.sum(pattern, axis=-2, keepdims=True)
    full = (*independent, K, N)
    if _lib.is_torch(Y):
        return _lib.torch().from_numpy(pattern).to(Y.device).expand(full)
    return np.broadcast_to(pattern, full)
