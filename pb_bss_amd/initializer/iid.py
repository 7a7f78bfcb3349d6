"""Independent and identically distributed initialisations (reference: pb_bss/initializer/iid.py).

Every function maps an observation `Y` (..., N, D) to affiliations (..., K, N); only the shape of
`Y` is used.  With `permutation_free` ONE (K, N) draw is shared by all independent axes (a
read-only broadcast view, as in the reference).  A NumPy `Y` gives a NumPy array, a device tensor
a device tensor.

Where the numbers come from follows `pb_bss_amd.distribution.utils.set_random_init` /
PBBSS_RANDOM_INIT: 'numpy' (default) consumes NumPy's global generator call for call like the
reference, so a script seeded with np.random.seed sees the reference's numbers; 'device' draws
with torch's generator on the GPU (seed with torch.manual_seed).
"""
import numpy as np

from .. import _lib
from ..distribution import utils as _utils

__all__ = [
    'uniform_normalized',
    'dirichlet_uniform',
    'dirichlet',
    'one_hot',
]


def _shapes(Y, num_classes, permutation_free):
    """(shape of the draw, shape of the result)"""
    full = (*Y.shape[:-2], int(num_classes), Y.shape[-2])
    return (full[-2:] if permutation_free else full), full


def _on_device():
    return _utils._random_init == 'device'


def _draw_device(Y):
    """torch device the draw happens on"""
    t = _lib.torch()
    if _lib.is_torch(Y):
        return Y.device
    if _on_device():
        _lib.require_gpu()
        return t.device('cuda', t.cuda.current_device())
    return t.device('cpu')


def _finish(x, Y, full):
    """draw (torch tensor or NumPy array) -> broadcast result of the kind of Y"""
    t = _lib.torch()
    if _lib.is_torch(Y):
        if not _lib.is_torch(x):
            x = t.from_numpy(np.ascontiguousarray(x)).to(Y.device)
        return x.expand(full)
    if _lib.is_torch(x):
        x = x.cpu().numpy()
    return np.broadcast_to(x, full)


def uniform_normalized(
        Y,
        num_classes: int,
        permutation_free: bool = False,
):
    """Uniform draws normalised over the classes: the `num_classes=` initialisation of the
    trainers (`random_affiliation`)."""
    draw, full = _shapes(Y, num_classes, permutation_free)
    return _finish(_utils.random_affiliation(draw, _draw_device(Y)), Y, full)


def dirichlet_uniform(Y, num_classes, permutation_free=False):
    """dirichlet with alpha = 1: uniform on the probability simplex."""
    return dirichlet(Y, num_classes, permutation_free, alpha=1)


def dirichlet(
        Y,
        num_classes: int,
        permutation_free: bool = False,
        alpha=1,
):
    """Symmetric Dirichlet(alpha) affiliations, independent per observation."""
    assert np.isscalar(alpha), alpha
    draw, full = _shapes(Y, num_classes, permutation_free)
    K = int(num_classes)
    batch = (*draw[:-2], draw[-1])  # one K-vector per observation
    if _on_device():
        t = _lib.torch()
        conc = t.full((*batch, K), float(alpha), dtype=t.float64, device=_draw_device(Y))
        g = t._standard_gamma(conc)
        x = (g / g.sum(-1, keepdim=True)).transpose(-1, -2)
    else:
        x = np.swapaxes(np.random.dirichlet(np.full(K, alpha), size=batch), -1, -2)
    return _finish(x, Y, full)


def one_hot(
        Y,
        num_classes: int,
        permutation_free: bool = False,
):
    """Every observation belongs to one uniformly drawn class."""
    draw, full = _shapes(Y, num_classes, permutation_free)
    K = int(num_classes)
    batch = (*draw[:-2], draw[-1])
    if _on_device():
        t = _lib.torch()
        dev = _draw_device(Y)
        labels = t.randint(K, batch, device=dev)
        x = (labels[..., None, :] == t.arange(K, device=dev)[:, None]).to(t.float64)
    else:
        labels = np.random.randint(K, size=batch)
        x = (labels[..., None, :] == np.arange(K)[:, None]).astype(np.float64)
    return _finish(x, Y, full)
