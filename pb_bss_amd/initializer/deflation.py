"""Deterministic deflation seed (reference: pb_bss/initializer/deflation.py:6-89) on the device.

Class after class, the most salient frames -- per bin, or for the utterance as a whole
(`permutation_free`) -- give a local spatial covariance; every frame's squared cosine to its
principal eigenvector is the class posterior, and the saliencies are deflated by it.  The whole
seed is one call into csrc/initializer.hip (`pbbss_deflation_seed`); nothing is computed on the
host.
"""
from .. import _lib, engine
from ..distribution.utils import as_result


def _device_complex(Y):
    t = _lib.torch()
    name = str(Y.dtype).rsplit('.', 1)[-1]
    return _lib.to_device(Y, t.complex64 if name == 'complex64' else t.complex128)


def deflationSeed(
        Y,
        sources: int,
        saliencies=None,
        permutation_free: bool = True,
        neighbors: int = 5,
        similarity_transform=None,
        eps=0,
):
    """
    Args:
        Y: (..., F, T, D) complex, NumPy array or device tensor.  Leading axes are independent
            utterances (an extension over the reference, which takes (F, T, D)): each has its
            own cross-bin peak, the batch is one call.
        sources: number of classes K (2 <= K <= 19)
        saliencies: (..., F, T), default |Y[f, t, :]|
        permutation_free: one peak frame per utterance (arg-max of the saliency averaged over
            the bins) instead of one per bin
        neighbors: the local covariance spans 2 * neighbors + 1 frames around the peak
        similarity_transform: callable (similarity, saliencies) -> similarity, applied in every
            round; gets arrays of the caller's kind.  The rounds then run one by one.
        eps: floor of the posteriors before the class normalisation

    Returns:
        (..., K, F, T) float64, of the kind of `Y`.  complex64 observations are widened
        exactly; all arithmetic is float64.
    """
    t = _lib.require_gpu()
    like_torch = _lib.is_torch(Y)
    *lead, F, T, D = tuple(Y.shape)
    assert F in [257, 513], F
    assert T > 2 * neighbors, (T, neighbors)
    K = int(sources)
    y = _device_complex(Y).reshape(-1, F, T, D)
    B = y.shape[0]
    sal = None
    if saliencies is not None:
        assert tuple(saliencies.shape) == (*lead, F, T), (tuple(saliencies.shape), (*lead, F, T))
        sal = _lib.to_device(saliencies, t.float64).to(y.device).reshape(B, F, T)
    common = dict(saliency=sal, permutation_free=permutation_free, neighbors=neighbors, eps=eps)
    if similarity_transform is None:
        out = engine.deflation_seed(y, K, **common)
    else:
        def user(x):  # (B, F, T) device -> what the caller's transform works with
            return as_result(x.reshape(*lead, F, T), like_torch)

        out = t.empty((B, K, F, T), dtype=t.float64, device=y.device)
        state = t.empty((B, F, T), dtype=t.float64, device=y.device)
        engine.deflation_seed(y, K, rounds=(0, 0), finalize=False, state=state, out=out, **common)
        for r in range(K - 1):
            before = state.clone()
            engine.deflation_seed(y, K, rounds=(r, r + 1), finalize=False, state=state, out=out,
                                  **common)
            similarity = similarity_transform(user(out[:, r]), user(before))
            similarity = _lib.to_device(similarity, t.float64).to(y.device).reshape(B, F, T)
            out[:, r] = similarity
            state = (before * (1 - similarity)).contiguous()
        engine.deflation_seed(y, K, rounds=(K - 1, K - 1), finalize=True, state=state, out=out,
                              **common)
    return as_result(out.reshape(*lead, K, F, T), like_torch)
