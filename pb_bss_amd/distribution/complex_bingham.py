"""Complex Bingham distribution on the device.

Mirrors pb_bss/distribution/complex_bingham.py: `ComplexBingham` (covariance eigenvectors and
eigenvalues; covariance, pdf, log_pdf, log_norm, norm, _remove_duplicate_eigenvalues) and
`ComplexBinghamTrainer` (fit / _fit / find_eigenvalues_v3).  The parameter solve and the
normaliser run in the HIP kernels of csrc/cbmm.hpp: c(lam) = 2 pi^D e[lam], the divided
difference of exp by scaling and squaring (stable at any eigenvalue spacing), and the bounded
Gauss-Newton solve of grad ln c(lam) = s iterated to rounding level (the reference stops
scipy's least_squares at its default tolerances).  The sympy helpers of the reference
(find_eigenvalues_sympy, grad_log_norm_symbolic) are not ported.
"""
from dataclasses import dataclass

import numpy as np

from .. import _lib, engine
from .utils import _ProbabilisticModel, as_result
from .complex_watson import normalize_observation  # noqa: F401  (reference :12-25)

__all__ = ['ComplexBingham', 'ComplexBinghamTrainer', 'normalize_observation', 'force_hermitian']

MAX_DIMENSION = 8  # sensors served by the kernels


def _check_dimension(D):
    if D > MAX_DIMENSION:
        raise NotImplementedError(
            f'complex Bingham: D = {D} sensors, the kernels serve D <= {MAX_DIMENSION}')


def force_hermitian(matrix):
    """(A + A^H) / 2 (reference :597-608)."""
    if _lib.is_torch(matrix):
        return (matrix + matrix.conj().transpose(-1, -2)) / 2
    return (matrix + np.swapaxes(matrix.conj(), -1, -2)) / 2


def _like(x, like_torch):
    return as_result(x, like_torch)


@dataclass
class ComplexBingham(_ProbabilisticModel):
    covariance_eigenvectors: np.ndarray = None  # (..., D, D)
    covariance_eigenvalues: np.ndarray = None  # (..., D)

    def __post_init__(self):
        if not _lib.is_torch(self.covariance_eigenvectors) and \
                self.covariance_eigenvectors is not None:
            self.covariance_eigenvectors = np.array(self.covariance_eigenvectors)
        if not _lib.is_torch(self.covariance_eigenvalues):
            self.covariance_eigenvalues = np.array(self.covariance_eigenvalues)

    @property
    def covariance(self):
        """V diag(lam) V^H (reference :38-45)."""
        V, lam = self.covariance_eigenvectors, self.covariance_eigenvalues
        if _lib.is_torch(V):
            t = _lib.torch()
            return t.einsum('...wx,...x,...zx->...wz', V, lam.to(V.dtype), V.conj())
        return np.einsum('...wx,...x,...zx->...wz', V, lam, V.conj(), optimize='greedy')

    def _device_model(self, device, indep):
        t = _lib.torch()
        V = _lib.to_device(self.covariance_eigenvectors, t.complex128).to(device)
        lam = _lib.to_device(self.covariance_eigenvalues, t.float64).to(device)
        D = lam.shape[-1]
        return (V.expand(*indep, D, D).reshape(-1, 1, D, D).contiguous(),
                lam.expand(*indep, D).reshape(-1, 1, D).contiguous())

    def log_pdf(self, y):
        """y (..., T, D) -> yH B y - ln c(lam), shape (..., T) (reference :60-79).  Like the
        reference, y is used as given (no normalisation)."""
        like_torch = _lib.is_torch(y)
        t = _lib.torch()
        y = _lib.to_device(np.asarray(y) if not like_torch else y)
        if not y.is_complex():
            y = y.to(t.complex128)
        *yi, T, D = y.shape
        _check_dimension(D)
        lam_shape = tuple(np.shape(self.covariance_eigenvalues)[:-1])
        indep = tuple(np.broadcast_shapes(tuple(yi), lam_shape))
        V, lam = self._device_model(y.device, indep)
        B = V.shape[0]
        yb = y.expand(*indep, T, D).reshape(B, T, D)
        # the kernel sees unit-norm frames: scale the quadratic form back by |y|^2, in float64
        # like the kernel's own norm (a complex64 observation is widened first)
        y64 = yb.to(t.complex128)
        n2 = y64.real ** 2 + y64.imag ** 2
        n2 = n2.sum(-1)
        r = engine.cbmm_fit(yb.contiguous(), 1, model=(V, lam, t.ones((B, 1), dtype=t.float64,
                                                                        device=y.device)),
                            iterations=0, want_log_pdf=True)
        lnc = self._log_norm_device(V, lam)
        lp = (r['log_pdf'][:, 0] + lnc[:, None]) * n2 - lnc[:, None]
        return _like(lp.reshape(*indep, T), like_torch)

    def pdf(self, y):
        lp = self.log_pdf(y)
        return lp.exp() if _lib.is_torch(lp) else np.exp(lp)

    @staticmethod
    def _log_norm_device(V, lam, eps=1e-8):
        """ln c of a given model: the kernel's model set-up (iterations = 0) writes it out; a
        one-frame observation is all the launch needs."""
        t = _lib.torch()
        B, _, D = lam.shape
        y = t.zeros((B, 1, D), dtype=t.complex128, device=lam.device)
        y[..., 0] = 1.0
        r = engine.cbmm_fit(y, 1, model=(V, lam, t.ones((B, 1), dtype=t.float64,
                                                         device=lam.device)),
                            iterations=0, norm_eps=eps)
        return r['log_norm'][:, 0]

    def log_norm(self, remove_duplicate_eigenvalues=True, eps=1e-8):
        """ln c(lam) (reference :81-82, :84-186), computed stably as the divided difference of exp
        (csrc/cbmm.hpp).  remove_duplicate_eigenvalues: spaced >= eps first, as the reference;
        without it the divided difference of the eigenvalues as given (the reference's closed
        form loses its digits there, this one does not)."""
        lam = self.covariance_eigenvalues
        like_torch = _lib.is_torch(lam)
        t = _lib.torch()
        lam_d = _lib.to_device(lam, t.float64)
        D = lam_d.shape[-1]
        _check_dimension(D)
        indep = tuple(lam_d.shape[:-1])
        V = t.eye(D, dtype=t.complex128, device=lam_d.device).expand(*indep, D, D)
        lnc = self._log_norm_device(V.reshape(-1, 1, D, D).contiguous(),
                                    lam_d.reshape(-1, 1, D).contiguous(),
                                    eps if remove_duplicate_eigenvalues else 0.0)
        return _like(lnc.reshape(indep), like_torch)

    def norm(self, remove_duplicate_eigenvalues=True, eps=1e-8):
        lnc = self.log_norm(remove_duplicate_eigenvalues, eps)
        return lnc.exp() if _lib.is_torch(lnc) else np.exp(lnc)

    @classmethod
    def _remove_duplicate_eigenvalues(cls, covariance_eigenvalues, eps=1e-8):
        """(inverse permutation, sorted eigenvalues spaced >= eps) (reference :188-224).
        A host helper on small arrays (ties keep their order)."""
        ev = np.asarray(covariance_eigenvalues, dtype=np.float64)
        perm = np.argsort(ev, axis=-1, kind='stable')
        srt = np.take_along_axis(ev, perm, axis=-1).copy()
        diff = np.maximum(np.diff(srt, axis=-1), eps)
        srt[..., 1:] = srt[..., 0][..., None] + np.cumsum(diff, axis=-1)
        inverse_permutation = np.arange(perm.shape[-1])[np.argsort(perm, axis=-1)]
        return inverse_permutation, srt


class ComplexBinghamTrainer:
    def __init__(self, dimension=None, max_concentration=np.inf, eignevalue_eps=1e-8):
        """The reference's (misspelled) keyword `eignevalue_eps` is kept (reference :227-242)."""
        self.dimension = dimension
        assert max_concentration > 0, max_concentration
        self.max_concentration = max_concentration
        self.eignevalue_eps = eignevalue_eps

    @classmethod
    def find_eigenvalues_v3(cls, scatter_eigenvalues, eps=1e-8, max_concentration=np.inf):
        """Bingham eigenvalues lam (max 0) with grad ln c(lam) = s, for (..., D) scatter
        eigenvalues in any order (reference :304-396), on the device."""
        like_torch = _lib.is_torch(scatter_eigenvalues)
        t = _lib.torch()
        s = _lib.to_device(scatter_eigenvalues if like_torch
                           else np.asarray(scatter_eigenvalues, dtype=np.float64), t.float64)
        D = s.shape[-1]
        _check_dimension(D)
        lam, _ = engine.cbingham_find_eigenvalues(s.reshape(-1, D).contiguous(), eps,
                                                  max_concentration)
        return _like(lam.reshape(s.shape), like_torch)

    # the same equations (reference :245-301); one solver serves both
    find_eigenvalues_v2 = find_eigenvalues_v3

    def fit(self, y, saliency=None) -> ComplexBingham:
        """y (..., N, D) complex, saliency (..., N) (reference :549-569)."""
        like_torch = _lib.is_torch(y)
        assert (y.is_complex() if like_torch else np.iscomplexobj(y)), y.dtype
        assert y.shape[-1] > 1
        if self.dimension is None:
            self.dimension = y.shape[-1]
        else:
            assert self.dimension == y.shape[-1], (
                'You initialized the trainer with a different dimension than '
                'you are using to fit a model. Use a new trainer, when you '
                'change the dimension.')
        return self._fit(y, saliency=saliency)

    def _fit(self, y, saliency) -> ComplexBingham:
        """Weighted scatter -> eigh -> parameter solve (reference :571-594), one fused M-step
        of the EM kernel (iterations = 1 from the saliency as the affiliation).  The kernel
        unit-normalises the frames on load; the reference's _fit receives them normalised by
        fit(), so both agree on every input fit() passes (only a direct _fit call with raw
        frames would differ)."""
        like_torch = _lib.is_torch(y)
        t = _lib.torch()
        y = _lib.to_device(y)
        *indep, N, D = y.shape
        _check_dimension(D)
        indep = tuple(indep)
        if saliency is None:
            w = t.ones((*indep, N), dtype=t.float64, device=y.device)
        else:
            w = _lib.to_device(saliency, t.float64).to(y.device)
            indep = tuple(np.broadcast_shapes(indep, tuple(w.shape[:-1])))
            w = w.expand(*indep, N)
        yb = y.expand(*indep, N, D).reshape(-1, N, D).contiguous()
        B = yb.shape[0]
        r = engine.cbmm_fit(yb, 1, gamma0=w.reshape(B, 1, N).contiguous(), iterations=1,
                            max_concentration=self.max_concentration,
                            eigenvalue_eps=self.eignevalue_eps)
        return ComplexBingham(
            covariance_eigenvectors=_like(r['eigvec'].reshape(*indep, D, D), like_torch),
            covariance_eigenvalues=_like(r['eigval'].reshape(*indep, D), like_torch))
