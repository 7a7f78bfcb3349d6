"""Complex circular-symmetric Gaussian of a sensor vector on the device.

Mirrors pb_bss/distribution/complex_circular_symmetric_gaussian.py: same class names, argument
meaning, shapes and error behaviour; `log_pdf` and `fit` call the HIP library (csrc/ccsg.hip)
instead of NumPy/LAPACK.  The arithmetic is float64 on the exactly widened values: results are
those of the reference on `y.astype(complex128)`.

The one deviation: `log_pdf` factors the covariance by Cholesky, so a Hermitian matrix that is
indefinite raises `np.linalg.LinAlgError` like a singular one, where the reference's LU returns
numbers (a "density" with a negative quadratic form).  Only the lower triangle and the real
part of the diagonal of a covariance are read.
"""
from dataclasses import dataclass

import numpy as np

from .. import _lib, engine
from .utils import _ProbabilisticModel, as_result, reference_single, to_single
from ..utils import is_broadcast_compatible

__all__ = ['ComplexCircularSymmetricGaussian', 'ComplexCircularSymmetricGaussianTrainer']


def _complex_device(y):
    t = _lib.torch()
    y = _lib.to_device(y)
    if y.dtype not in (t.complex64, t.complex128):
        raise AssertionError(y.dtype)  # reference: assert np.iscomplexobj(y)
    return y


def _fold(y_indep, p_indep):
    """Independent axes of y against those of a per-class parameter -> (lead, K, y_lead, mixture):
    K is the trailing parameter axis that the observation does not have (size 1 or missing), the
    batch is everything else (as ComplexAngularCentralGaussian._device_log_pdf folds it)."""
    full = tuple(np.broadcast_shapes(y_indep, p_indep))
    if len(full) >= 1 and (len(y_indep) == 0 or y_indep[-1] == 1) and len(p_indep) >= 1:
        return full[:-1], full[-1], tuple(y_indep[:-1]), True
    return full, 1, tuple(y_indep), False


@dataclass
class ComplexCircularSymmetricGaussian(_ProbabilisticModel):
    covariance: np.ndarray = None  # (..., D, D)

    def log_pdf(self, y):
        """y (..., N, D) -> (..., N), the independent axes broadcast against those of the
        covariance (reference :26-48); y (F, 1, N, D) against covariance (F, K, D, D) is one call
        with the class axis.  A covariance that is not positive definite raises
        np.linalg.LinAlgError; a NaN in a covariance gives NaN for that covariance only."""
        like_torch = _lib.is_torch(y)
        t = _lib.torch()
        single = reference_single(y, self.covariance)
        y = _complex_device(y)
        cov = _lib.to_device(self.covariance, t.complex128).to(y.device)
        *indep, N, D = y.shape
        assert cov.shape[-2:] == (D, D), (cov.shape, y.shape)
        lead, K, y_lead, mixture = _fold(tuple(indep), tuple(cov.shape[:-2]))
        B = int(np.prod(lead)) if lead else 1
        yb = y.reshape(*y_lead, N, D).expand(*lead, N, D).reshape(B, N, D).contiguous()
        shape = (*lead, K) if mixture else lead
        cb = cov.expand(*shape, D, D).reshape(B, K, D, D).contiguous()
        log_pdf, _, status = engine.ccsg_log_pdf(yb, cb)
        if engine._status_bits(status) & _lib.ST_NOT_POSDEF:
            raise np.linalg.LinAlgError('Singular matrix (covariance not positive definite)')
        out = log_pdf.reshape(*shape, N)
        return as_result(to_single(out) if single else out, like_torch)

    def sample(self, size):
        """`size` (...,) -> (..., D) draws (reference :50-72).  Host side: NumPy's global
        generator, real parts before imaginary parts, so a seeded run reproduces the reference's
        draws."""
        cov = self.covariance
        cov = np.asarray(_lib.to_host(cov) if _lib.is_torch(cov) else cov)
        if cov.ndim > 2:
            raise NotImplementedError(
                "Not quite clear how the correct broadcasting would look like.")
        D = cov.shape[-1]
        real = np.random.normal(size=(*size, D))
        imag = np.random.normal(size=(*size, D))
        x = real + 1j * imag
        x /= np.sqrt(2)
        cholesky = np.linalg.cholesky(cov)
        return (cholesky @ x.T).T


class ComplexCircularSymmetricGaussianTrainer:
    def fit(self, y, saliency=None, covariance_type="full"):
        """y (..., N, D) complex, saliency (..., N) or None (reference :76-92); saliency
        (..., K, N) against y (..., 1, N, D) gives covariance (..., K, D, D) in one call."""
        if not _lib.is_torch(y):
            y = np.asarray(y)
            assert np.iscomplexobj(y), y.dtype
        if saliency is not None:
            assert is_broadcast_compatible(tuple(y.shape[:-1]), tuple(saliency.shape)), (
                y.shape, saliency.shape)
        return self._fit(y, saliency=saliency, covariance_type=covariance_type)

    def _fit(self, y, saliency, covariance_type):
        if covariance_type != "full":
            raise ValueError(f"Unknown covariance type '{covariance_type}'.")
        like_torch = _lib.is_torch(y)
        t = _lib.torch()
        single = reference_single(y, saliency)
        y = _complex_device(y)
        *indep, N, D = y.shape
        if saliency is None:
            lead, K, y_lead, mixture = tuple(indep), 1, tuple(indep), False
            sb = None
        else:
            sal = _lib.to_device(saliency).to(y.device)
            if sal.dtype not in (t.float32, t.float64):
                sal = sal.to(t.float64)
            lead, K, y_lead, mixture = _fold(tuple(indep), tuple(sal.shape[:-1]))
        B = int(np.prod(lead)) if lead else 1
        shape = (*lead, K) if mixture else lead
        if saliency is not None:
            sb = sal.expand(*shape, N).reshape(B, K, N).contiguous()
        yb = y.reshape(*y_lead, N, D).expand(*lead, N, D).reshape(B, N, D).contiguous()
        cov = engine.ccsg_fit(yb, sb).reshape(*shape, D, D)
        return ComplexCircularSymmetricGaussian(
            covariance=as_result(to_single(cov) if single else cov, like_torch))
