"""Gaussian mixture model on real embeddings on the HIP embedding kernels.
Mirrors pb_bss/distribution/gmm.py:16-171: `GMM` (weight, gaussian; predict) and
`GMMTrainer` (fit / fit_predict) for covariance_type 'full' (the reference's default;
FP64 matrix-pipe kernels of csrc/gauss_full.hip, D <= 63) and 'spherical' (the covariance
model the joint GCACGMM uses, gcacgmm.py:141; the vMF mixture's E-step / M-step kernels on the
raw embedding): the whole EM loop is one C-ABI call (`pbbss_gmm_full_fit` / `pbbss_gmm_fit`).
covariance_type 'diagonal' and the `weight_constant_axis` sets beyond (-1,), (-2,), -2 run the
reference's loop step by step on the device (`_embed_stepwise.py`: log-pdf, softmax, weight and
single-Gaussian fit kernels, no host round trip inside the loop).  `BinaryGMM` and
`BinaryGMMTrainer` (:176-230, k-means through sklearn in the reference) live in kmeans.py on the
kernels of csrc/kmeans.hip and are exported from here as in the reference module.
"""
from dataclasses import dataclass

import numpy as np

from .. import _lib, engine
from . import _embed_stepwise as sw
from . import _mixture as mix
from .gaussian import DiagonalGaussian, Gaussian, SphericalGaussian
from .kmeans import BinaryGMM, BinaryGMMTrainer, KMeans  # noqa: F401  (KMeans: the name gmm.py imports)
from .utils import _ProbabilisticModel, as_result
from ..utils import labels_to_one_hot  # noqa: F401  (names the reference module exposes)
from .gaussian import GaussianTrainer  # noqa: F401  (names the reference module exposes)
from .mixture_model_utils import estimate_mixture_weight, log_pdf_to_affiliation  # noqa: F401  (names the reference module exposes)

__all__ = ['GMM', 'GMMTrainer', 'BinaryGMM', 'BinaryGMMTrainer']


_CLASS, _UNIFORM, _ONES = _lib.WEIGHT_PER_CLASS_MEAN, _lib.WEIGHT_UNIFORM, mix.WEIGHT_ONES


def _weight_kind(weight_constant_axis, ndim):
    """How estimate_mixture_weight (mixture_model_utils.py:133-203) is driven:
    (-1,) / -1: per-class weights (K, 1); int -2: the constant 1/K (:180-183);
    tuple (-2,) -- the default of fit_predict --: the general path averages over the class
    axis and L1-normalises along it, i.e. a (1, N) array of ones (:192-201).  Weights that
    are constant over the classes cancel in the posterior, so both run as the uniform mode.
    None: any other axis set, the step-wise device loop (_embed_stepwise.py)."""
    return mix.fused_weight_mode(weight_constant_axis, ndim, ones=True)


def _check_covariance_type(covariance_type):
    if covariance_type not in ('spherical', 'diagonal', 'full'):
        raise ValueError(f"Unknown covariance type '{covariance_type}'.")  # gaussian.py:184


_CLS = {'full': Gaussian, 'diagonal': DiagonalGaussian, 'spherical': SphericalGaussian}


def _kind_of(gaussian):
    for name, cls in _CLS.items():
        if type(gaussian) is cls:
            return name
    raise TypeError(type(gaussian))


@dataclass
class GMM(_ProbabilisticModel):
    weight: np.ndarray = None  # (..., K, 1)
    gaussian: object = None  # Gaussian (full covariance) or SphericalGaussian

    def predict(self, x):
        """x (..., N, D) real -> affiliations (..., K, N) (:21-25)."""
        like_torch = _lib.is_torch(x)
        t = _lib.torch()
        x = _lib.to_device(x)
        assert not x.is_complex(), x.dtype
        *indep, N, E = x.shape
        K = self.gaussian.mean.shape[-2]
        kind = _kind_of(self.gaussian)
        full = kind == 'full'
        cs = mix.covariance_shape(kind, E)
        mean = mix.flatten_param(self.gaussian.mean, indep, (K, E), t.float64, x.device)
        cov = mix.flatten_param(self.gaussian.covariance, indep, (K, *cs), t.float64, x.device)
        w = _lib.to_device(self.weight, t.float64).to(x.device)
        general = kind == 'diagonal' or (w.shape[-1] != 1 and w.shape[-2] != 1) or (
            w.ndim > 2 and any(a != 1 for a in w.shape[:-2]) and w.shape[-1] != 1)
        if general:
            # diagonal covariances / weights that vary over classes AND frames: the general
            # log-pdf + softmax steps
            aff = sw.affiliation(kind, x.reshape(-1, N, E), mean, cov, w, tuple(indep))
            return as_result(aff.reshape(*indep, K, N), like_torch)
        if w.shape[-1] != 1:
            # (..., 1, N): constant over the classes (weight_constant_axis=(-2,)), cancels in
            # the posterior (mixture_model_utils.py:37-47) -- evaluated with uniform weights
            if w.shape[-2] != 1:
                raise NotImplementedError(f'frame-dependent class weights {tuple(w.shape)}')
            w = mix.uniform_weight(K, x.device)
        model = (mean, cov, mix.flatten_param(w, indep, (K, 1), t.float64).reshape(-1, K))
        if full:
            r = engine.gmm_full_fit(x.reshape(-1, N, E), K, model=model, iterations=0,
                                    final_predict=True)
            if int(r['status'].item()) != 0:
                raise mix.not_positive_definite()
        else:
            r = engine.gmm_fit(x.reshape(-1, N, E), K, model=model, iterations=0,
                               final_predict=True)
        return as_result(r['affiliation'].reshape(*indep, K, N), like_torch)


class GMMTrainer:
    def __init__(self, eps=1e-10):
        self.eps = eps
        self.log_likelihood_history = []

    def fit(self, y, initialization=None, num_classes=None, iterations=100, *, saliency=None,
            weight_constant_axis=(-1,), covariance_type='full', fixed_covariance=None):
        """y (..., N, D) real; initialization (..., K, N); saliency (..., N);
        fixed_covariance (..., K) (:33-95)."""
        _check_covariance_type(covariance_type)
        p = mix.prepare_fit(y, initialization, num_classes, saliency, weight_constant_axis,
                            complex_input=False)
        y, indep, N, E, K, like_torch = p.y, p.indep, p.N, p.D, p.K, p.like_torch
        t = _lib.torch()
        kind = _weight_kind(p.weight_constant_axis, p.ndim)
        # the fused loops serve 'spherical' and 'full' with the class-wise / uniform weights
        stepwise = kind is None or covariance_type == 'diagonal'
        full = covariance_type == 'full'
        cs = mix.covariance_shape(covariance_type, E)
        sal = p.saliency  # None: ones (:79-80), which the kernels assume anyway
        if sal is not None and not stepwise and kind == _ONES \
                and not bool((sal > 0).all().item()):
            raise NotImplementedError(
                'weight_constant_axis=(-2,) with zero saliency entries (zero weights)')
        fixed = None
        if fixed_covariance is not None:
            fixed = _lib.to_device(fixed_covariance, t.float64).to(y.device)
            assert tuple(fixed.shape) == (*indep, K, *cs), (
                f'{tuple(fixed.shape)} != {(*indep, K, *cs)}')  # :161-163
        if iterations <= 0:
            return None  # the reference's loop body never runs (:127-141)
        if stepwise:
            r = sw.fit(covariance_type, y, p.gamma0, iterations, sal, p.weight_constant_axis,
                       fixed_scale=fixed)
            weight, cov = r['weight'], r['scale']
        else:
            if fixed is not None:
                fixed = fixed.reshape(-1, K, *cs).contiguous()
            fit = engine.gmm_full_fit if full else engine.gmm_fit
            r = fit(y.reshape(-1, N, E), K, gamma0=p.gamma0.reshape(-1, K, N).contiguous(),
                    iterations=iterations, saliency=sal,
                    weight_mode=_lib.WEIGHT_PER_CLASS_MEAN if kind == _CLASS
                    else _lib.WEIGHT_UNIFORM, fixed_covariance=fixed)
            if full and int(r['status'].item()) != 0:
                raise mix.not_positive_definite()
            if kind == _ONES:
                weight = t.ones((*indep, 1, N), dtype=t.float64, device=y.device)
            else:
                weight = mix.fused_weight(kind, r['weight'], indep, K, y.device)
            cov = r['covariance']
        return GMM(
            weight=as_result(weight, like_torch),
            gaussian=_CLS[covariance_type](
                mean=as_result(r['mean'].reshape(*indep, K, E), like_torch),
                covariance=as_result(cov.reshape(*indep, K, *cs), like_torch)))

    def fit_predict(self, y, initialization=None, num_classes=None, iterations=100, *,
                    saliency=None, weight_constant_axis=(-2,), covariance_type='full',
                    fixed_covariance=None):
        """Fit a model. Then just return the posterior affiliations (:97-119)."""
        model = self.fit(y=y, initialization=initialization, num_classes=num_classes,
                         iterations=iterations, saliency=saliency,
                         weight_constant_axis=weight_constant_axis,
                         covariance_type=covariance_type, fixed_covariance=fixed_covariance)
        return model.predict(y)
