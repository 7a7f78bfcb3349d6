"""Complex-Watson mixture model and EM trainer backed by the persistent HIP
kernel `cwmm_em_kernel` (csrc/cwmm.hpp).

Mirrors pb_bss/distribution/cwmm.py: `CWMM` (weight, complex_watson; predict)
and `CWMMTrainer` (fit / fit_predict) with the reference's arguments and
assertions.  Fused single-launch path for weight_constant_axis in
{(-1,), -1, -2} without an inline aligner; options that couple frequency bins
run E- and M-steps per iteration with the host hook in between (same entry
point with iterations = 0 / 1).
"""
from dataclasses import dataclass
from functools import cached_property

import numpy as np

from .. import _lib, engine
from . import _mixture as mix
from .complex_watson import ComplexWatson, ComplexWatsonTrainer
from .mixture_model_utils import (  # noqa: F401  (re-exported like the reference's cwmm.py)
    apply_inline_permutation_alignment,
    estimate_mixture_weight,
    log_pdf_to_affiliation,
)
from .complex_angular_central_gaussian import normalize_observation  # noqa: F401
from .utils import _ProbabilisticModel, as_result

__all__ = ['CWMM', 'CWMMTrainer']


def _components(complex_watson, indep, K, D, device):
    """-> mode (B, K, D) complex128, concentration (B, K) float64"""
    t = _lib.torch()
    return (mix.flatten_param(complex_watson.mode, indep, (K, D), t.complex128, device),
            mix.flatten_param(complex_watson.concentration, indep, (K,), t.float64, device))


def _unit_weight(yb, K):
    t = _lib.torch()
    return t.ones((yb.shape[0], K), dtype=t.float64, device=yb.device)


def _log_pdf(yb, K, mode, conc, ones_w):
    """Class log-pdfs (B, K, N): `pbbss_cwmm_fit` with iterations = 0 and unit weights."""
    return engine.cwmm_fit(yb, K, None, model=(mode, conc, ones_w), iterations=0,
                           want_log_pdf=True)['log_pdf']


@dataclass
class CWMM(_ProbabilisticModel):
    weight: np.ndarray = None  # (..., K, 1)
    complex_watson: ComplexWatson = None

    def predict(self, y):
        """y (..., N, D) -> affiliations (..., K, N) (reference :25-38; the
        observation is unit-normalised inside the kernel)."""
        like_torch = _lib.is_torch(y)
        t = _lib.torch()
        y = _lib.to_device(y)
        assert y.dtype in (t.complex64, t.complex128), y.dtype
        *indep, N, D = y.shape
        K = self.complex_watson.mode.shape[-2]
        yb = y.reshape(-1, N, D).contiguous()
        mode, conc = _components(self.complex_watson, indep, K, D, y.device)
        w = _lib.to_device(self.weight, t.float64).to(y.device)
        if w.shape[-1] != 1:
            # frame-varying weights (weight_constant_axis without -1, reference :40-52 with a
            # (..., K, N) weight): class log-pdfs, then the general softmax step
            aff = engine.log_pdf_to_affiliation(_log_pdf(yb, K, mode, conc, _unit_weight(yb, K)),
                                                mix.flatten_weight(w, indep))
            return as_result(aff.reshape(*indep, K, N), like_torch)
        wb = mix.flatten_param(w, indep, (K, 1), t.float64).reshape(-1, K)
        r = engine.cwmm_fit(yb, K, None, model=(mode, conc, wb), iterations=0,
                            final_predict=True)
        return as_result(r['affiliation'].reshape(*indep, K, N), like_torch)

    _predict = predict  # the kernel normalises; already-normalised input is unchanged by it


class CWMMTrainer:
    def __init__(self, dimension=None, max_concentration=500, spline_markers=1000):
        self.dimension = dimension
        self.max_concentration = max_concentration
        self.spline_markers = spline_markers

    @cached_property
    def complex_watson_trainer(self):
        return ComplexWatsonTrainer(self.dimension, max_concentration=self.max_concentration,
                                    spline_markers=self.spline_markers)

    def fit(self, y, initialization=None, num_classes=None, iterations=100, *,
            saliency=None, weight_constant_axis=(-1,), affiliation_eps=0,
            inline_permutation_aligner=None):
        """EM for complex-Watson mixtures, any number of independent axes
        (reference :76-149).  y (..., T, D); initialization (..., K, T)."""
        assert affiliation_eps == 0, affiliation_eps  # reference :161
        p = mix.prepare_fit(y, initialization, num_classes, saliency, weight_constant_axis,
                            complex_input=True)
        indep, N, D, K, like_torch = p.indep, p.N, p.D, p.K, p.like_torch
        mix.check_dimension(self, D)
        yb = p.y.reshape(-1, N, D).contiguous()
        spline = self.complex_watson_trainer.device_spline(yb.device)
        gamma0 = p.gamma0.reshape(-1, K, N).contiguous()
        r = None
        if inline_permutation_aligner is None:
            wmode = mix.fused_weight_mode(p.weight_constant_axis, p.ndim)
            smode = mix.shared_weight_mode(p.weight_constant_axis, p.ndim)
            if wmode is not None:
                r = engine.cwmm_fit(yb, K, spline, gamma0=gamma0, iterations=iterations,
                                    saliency=p.saliency, weight_mode=wmode)
                weight = mix.fused_weight(wmode, r['weight'], indep, K, yb.device)
            elif smode is not None:
                # weights averaged over the bins of an utterance ((-3, -1), cwmm.py:217-240): one
                # cooperative launch (csrc/cwmm.hpp: WatsonShared); None: not served / timed out
                r = engine.cwmm_fit(yb, K, spline, gamma0=gamma0, iterations=iterations,
                                    saliency=p.saliency, group=indep[-1], weight_mode=smode)
                if r is not None:
                    weight = r['weight'].reshape(
                        *indep[:-1], 1, K, N if smode == _lib.WEIGHT_SHARED_KT else 1)
        if r is not None:
            mode, conc = r['mode'], r['concentration']
        else:
            # The reference loop (:151-182) for the options that couple the bins
            # (`weight_constant_axis` with independent axes, frame-varying weights, an inline
            # aligner): `pbbss_cwmm_fit` with iterations = 0 (class log-pdfs) and iterations = 1
            # (M-step) around the shared softmax / aligner / weight steps
            ones_w = _unit_weight(yb, K)

            def m_step(masked):
                r = engine.cwmm_fit(yb, K, spline, gamma0=masked, iterations=1)
                return r['mode'], r['concentration']

            (mode, conc), weight = mix.stepwise_em(
                p.gamma0, iterations, lambda model: _log_pdf(yb, K, *model, ones_w), m_step,
                saliency=p.saliency, weight_constant_axis=p.weight_constant_axis,
                aligner=inline_permutation_aligner)
        return CWMM(weight=as_result(weight, like_torch),
                    complex_watson=ComplexWatson(
                        mode=as_result(mode.reshape(*indep, K, D), like_torch),
                        concentration=as_result(conc.reshape(*indep, K), like_torch)))

    def fit_predict(self, y, initialization=None, num_classes=None, iterations=100, *,
                    saliency=None, weight_constant_axis=(-1,), affiliation_eps=0,
                    inline_permutation_aligner=None):
        """Fit a model, then return the posterior affiliations (reference :184-210)."""
        model = self.fit(y=y, initialization=initialization, num_classes=num_classes,
                         iterations=iterations, saliency=saliency,
                         weight_constant_axis=weight_constant_axis,
                         affiliation_eps=affiliation_eps,
                         inline_permutation_aligner=inline_permutation_aligner)
        return model.predict(y)
