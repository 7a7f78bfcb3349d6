"""von Mises-Fisher mixture model (clustering of unit-norm embeddings) on the HIP
embedding kernels.  Mirrors pb_bss/distribution/vmfmm.py:14-172: `VMFMM`
(vmf, weight; predict) and `VMFMMTrainer` (fit / fit_predict).

The whole EM loop is one C-ABI call (`pbbss_vmfmm_fit`): per iteration one
E-step kernel over the transposed embedding and one M-step reduction over the
row-major embedding, enqueued back to back on the caller's stream.
"""
from dataclasses import dataclass

import numpy as np

from .. import _lib, engine
from . import _embed_stepwise as sw
from . import _mixture as mix
from .utils import _ProbabilisticModel, as_result
from .von_mises_fisher import VonMisesFisher
from .von_mises_fisher import VonMisesFisherTrainer  # noqa: F401  (names the reference module exposes)
from .mixture_model_utils import estimate_mixture_weight, log_pdf_to_affiliation  # noqa: F401  (names the reference module exposes)

__all__ = ['VMFMM', 'VMFMMTrainer']


@dataclass
class VMFMM(_ProbabilisticModel):
    vmf: VonMisesFisher = None
    weight: np.ndarray = None  # (..., K, 1)

    def predict(self, y):
        """y (..., N, D) real -> affiliations (..., K, N) (:19-31)."""
        like_torch = _lib.is_torch(y)
        t = _lib.torch()
        y = _lib.to_device(y)
        assert not y.is_complex(), y.dtype
        *indep, N, E = y.shape
        K = self.vmf.mean.shape[-2]
        mean = mix.flatten_param(self.vmf.mean, indep, (K, E), t.float64, y.device)
        conc = mix.flatten_param(self.vmf.concentration, indep, (K,), t.float64, y.device)
        w = _lib.to_device(self.weight, t.float64).to(y.device)
        if w.shape[-1] != 1 or (w.ndim > 2 and tuple(w.shape[:-2]) != tuple(indep)
                                and any(a != 1 for a in w.shape[:-2])):
            # frame-varying weights (weight_constant_axis without -1): the general softmax step
            aff = sw.affiliation('vmf', y.reshape(-1, N, E), mean, conc, w, tuple(indep))
            return as_result(aff.reshape(*indep, K, N), like_torch)
        model = (mean, conc, mix.flatten_param(w, indep, (K, 1), t.float64).reshape(-1, K))
        r = engine.vmfmm_fit(y.reshape(-1, N, E), K, model=model, iterations=0,
                             final_predict=True)
        return as_result(r['affiliation'].reshape(*indep, K, N), like_torch)

    _predict = predict  # normalising unit rows again is the identity


class VMFMMTrainer:
    """The vMFMM can be used to cluster the embeddings."""

    def fit(self, y, initialization=None, num_classes=None, iterations=100, saliency=None,
            weight_constant_axis=(-1,), min_concentration=1e-10, max_concentration=500):
        """EM for vMFMMs with any number of independent dimensions (:42-104).
        y (..., N, D) real; initialization (..., K, N); saliency (..., N)."""
        p = mix.prepare_fit(y, initialization, num_classes, saliency, weight_constant_axis,
                            complex_input=False)
        y, indep, N, E, K, like_torch = p.y, p.indep, p.N, p.D, p.K, p.like_torch
        assert iterations > 0, iterations
        # any axis set but (-1,) / -1 / int -2: the step-wise device loop (_embed_stepwise.py)
        mode = mix.fused_weight_mode(p.weight_constant_axis, p.ndim)
        if mode is None:
            r = sw.fit('vmf', y, p.gamma0, iterations, p.saliency, p.weight_constant_axis,
                       min_concentration=min_concentration, max_concentration=max_concentration)
            weight, conc = r['weight'], r['scale']
        else:
            r = engine.vmfmm_fit(y.reshape(-1, N, E), K,
                                 gamma0=p.gamma0.reshape(-1, K, N).contiguous(),
                                 iterations=iterations, saliency=p.saliency, weight_mode=mode,
                                 min_concentration=min_concentration,
                                 max_concentration=max_concentration)
            weight = mix.fused_weight(mode, r['weight'], indep, K, y.device)
            conc = r['concentration']
        return VMFMM(
            weight=as_result(weight, like_torch),
            vmf=VonMisesFisher(
                mean=as_result(r['mean'].reshape(*indep, K, E), like_torch),
                concentration=as_result(conc.reshape(*indep, K), like_torch)))

    def fit_predict(self, y, initialization=None, num_classes=None, iterations=100,
                    saliency=None, weight_constant_axis=(-1,), min_concentration=1e-10,
                    max_concentration=500):
        """Fit a model. Then just return the posterior affiliations (:106-127)."""
        model = self.fit(y=y, initialization=initialization, num_classes=num_classes,
                         iterations=iterations, saliency=saliency,
                         min_concentration=min_concentration,
                         max_concentration=max_concentration,
                         weight_constant_axis=weight_constant_axis)
        return model.predict(y)
