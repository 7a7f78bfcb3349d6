"""Complex-Bingham mixture model and EM trainer backed by the persistent HIP
kernel `cbmm_em_kernel` (csrc/cbmm.hpp).

Mirrors pb_bss/distribution/cbmm.py: `CBMM` (weight, complex_bingham; predict)
and `CBMMTrainer` (fit / fit_predict) with the reference's arguments and
assertions.  Fused single-launch path for weight_constant_axis in
{(-1,), -1, -2} without an inline aligner and with affiliation_eps = 0; every
other option runs E- and M-steps per iteration on the device (same entry point
with iterations = 0 / 1, plus the softmax and weight kernels).
"""
from dataclasses import dataclass
from functools import cached_property

import numpy as np

from .. import _lib, engine
from . import _mixture as mix
from .complex_bingham import ComplexBingham, ComplexBinghamTrainer, normalize_observation  # noqa: F401
from .mixture_model_utils import (  # noqa: F401  (re-exported like the reference's cbmm.py)
    apply_inline_permutation_alignment,
    estimate_mixture_weight,
    log_pdf_to_affiliation,
)
from .utils import _ProbabilisticModel, as_result

__all__ = ['CBMM', 'CBMMTrainer']

MAX_CLASSES = 4  # classes served by the fused kernel


def _check_shape(D, K):
    if D > 8:
        raise NotImplementedError(f'CBMM: D = {D} sensors, the kernel serves D <= 8')
    if K > MAX_CLASSES:
        raise NotImplementedError(f'CBMM: K = {K} classes, the kernel serves K <= {MAX_CLASSES}')


def _log_pdf(yb, K, V, lam, ones_w):
    """Class log-pdfs (B, K, N): `pbbss_cbmm_fit` with iterations = 0 and unit weights."""
    return engine.cbmm_fit(yb, K, model=(V, lam, ones_w), iterations=0,
                           want_log_pdf=True)['log_pdf']


@dataclass
class CBMM(_ProbabilisticModel):
    weight: np.ndarray = None  # (..., K, 1)
    complex_bingham: ComplexBingham = None

    def predict(self, y, affiliation_eps=0):
        """y (..., N, D) -> affiliations (..., K, N) (reference :25-40; the observation is
        unit-normalised inside the kernel)."""
        like_torch = _lib.is_torch(y)
        t = _lib.torch()
        y = _lib.to_device(y)
        assert y.dtype in (t.complex64, t.complex128), y.dtype
        *indep, N, D = y.shape
        indep = tuple(indep)
        cb = self.complex_bingham
        K = cb.covariance_eigenvalues.shape[-2]
        _check_shape(D, K)
        V = mix.flatten_param(cb.covariance_eigenvectors, indep, (K, D, D), t.complex128, y.device)
        lam = mix.flatten_param(cb.covariance_eigenvalues, indep, (K, D), t.float64, y.device)
        B = V.shape[0]
        yb = y.reshape(-1, N, D).contiguous()
        w = _lib.to_device(self.weight, t.float64).to(y.device)
        if w.shape[-1] == 1 and affiliation_eps == 0:
            wb = mix.flatten_param(w, indep, (K, 1), t.float64).reshape(B, K)
            r = engine.cbmm_fit(yb, K, model=(V, lam, wb), iterations=0, final_predict=True)
            return as_result(r['affiliation'].reshape(*indep, K, N), like_torch)
        # frame-varying weights or a clipped softmax (reference :42-58): class log-pdfs, then the
        # general softmax step
        ones_w = t.ones((B, K), dtype=t.float64, device=y.device)
        aff = engine.log_pdf_to_affiliation(_log_pdf(yb, K, V, lam, ones_w),
                                            mix.flatten_weight(w, indep),
                                            affiliation_eps=affiliation_eps)
        return as_result(aff.reshape(*indep, K, N), like_torch)

    def _predict(self, y, affiliation_eps=0):
        return self.predict(y, affiliation_eps=affiliation_eps)  # normalising twice is harmless


class CBMMTrainer:
    def __init__(self, dimension=None, max_concentration=np.inf, eigenvalue_eps=1e-8):
        self.dimension = dimension
        self.max_concentration = max_concentration
        self.eigenvalue_eps = eigenvalue_eps

    @cached_property
    def complex_bingham_trainer(self):
        return ComplexBinghamTrainer(self.dimension, max_concentration=self.max_concentration,
                                     eignevalue_eps=self.eigenvalue_eps)

    def fit(self, y, initialization=None, num_classes=None, iterations=100, *,
            saliency=None, weight_constant_axis=(-1,), affiliation_eps=0,
            inline_permutation_aligner=None) -> CBMM:
        """EM for complex-Bingham mixtures, any number of independent axes
        (reference :79-167).  y (..., T, D); initialization (..., K, T)."""
        p = mix.prepare_fit(y, initialization, num_classes, saliency, weight_constant_axis,
                            complex_input=True)
        indep, N, D, K, like_torch = p.indep, p.N, p.D, p.K, p.like_torch
        t = _lib.torch()
        mix.check_dimension(self, D)
        _check_shape(D, K)
        yb = p.y.reshape(-1, N, D).contiguous()
        B = yb.shape[0]
        # the reference always passes a saliency, ones by default (:148-149)
        sal = p.saliency
        if sal is None:
            sal = t.ones((B, N), dtype=t.float64, device=yb.device)
        options = dict(max_concentration=self.max_concentration, eigenvalue_eps=self.eigenvalue_eps)
        mode = mix.fused_weight_mode(p.weight_constant_axis, p.ndim)
        if mode is not None and inline_permutation_aligner is None and affiliation_eps == 0:
            r = engine.cbmm_fit(yb, K, gamma0=p.gamma0.reshape(-1, K, N).contiguous(),
                                iterations=iterations, saliency=sal, weight_mode=mode, **options)
            V, lam = r['eigvec'], r['eigval']
            weight = mix.fused_weight(mode, r['weight'], indep, K, yb.device)
        else:
            # The reference loop (:181-203) for the options the fused kernel does not take
            # (weights shared over independent axes or frame-varying, an inline aligner, a
            # clipped softmax): `pbbss_cbmm_fit` with iterations = 0 (class log-pdfs) and
            # iterations = 1 (M-step) around the shared softmax / aligner / weight steps
            ones_w = t.ones((B, K), dtype=t.float64, device=yb.device)

            def m_step(masked):
                r = engine.cbmm_fit(yb, K, gamma0=masked, iterations=1, **options)
                return r['eigvec'], r['eigval']

            (V, lam), weight = mix.stepwise_em(
                p.gamma0, iterations, lambda model: _log_pdf(yb, K, *model, ones_w), m_step,
                saliency=sal, weight_constant_axis=p.weight_constant_axis,
                aligner=inline_permutation_aligner, affiliation_eps=affiliation_eps)
        return CBMM(
            weight=as_result(weight, like_torch),
            complex_bingham=ComplexBingham(
                covariance_eigenvectors=as_result(V.reshape(*indep, K, D, D), like_torch),
                covariance_eigenvalues=as_result(lam.reshape(*indep, K, D), like_torch)))

    def fit_predict(self, y, initialization=None, num_classes=None, iterations=100, *,
                    saliency=None, weight_constant_axis=(-1,), affiliation_eps=0,
                    inline_permutation_aligner=None):
        """Fit a model, then return the posterior affiliations (reference :151-171)."""
        model = self.fit(y=y, initialization=initialization, num_classes=num_classes,
                         iterations=iterations, saliency=saliency,
                         weight_constant_axis=weight_constant_axis,
                         affiliation_eps=affiliation_eps,
                         inline_permutation_aligner=inline_permutation_aligner)
        return model.predict(y)
