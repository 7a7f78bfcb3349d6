"""Host layer shared by the mixture trainers (cACGMM, cWMM, cBMM, vMFMM, GMM and the joint
models): everything between the reference-shaped `fit` / `predict` arguments and `engine.py`
that does not depend on the model family.

  * `weight_constant_axis` -> canonical axis set -> kernel weight mode
  * mixture weights on the device (`pbbss_estimate_mixture_weight`, host formula otherwise)
  * flattening the independent axes of parameters and weights for the C ABI
  * the argument preamble of `fit`
  * the step-wise EM loop and the aligner dispatch between its E- and M-step

Imports `_lib`, `engine` and `utils` only, so every trainer and `mixture_model_utils` can import
it at module level.
"""
from dataclasses import dataclass
from operator import xor

import numpy as np

from .. import _lib, engine
from .utils import random_affiliation

WEIGHT_ONES = 'ones'  # GMM: tuple (-2,), a (1, N) array of ones (see fused_weight_mode)


def covariance_shape(covariance_type, E):
    """Trailing shape of one class's covariance parameter (gaussian.py)."""
    return {'full': (E, E), 'diagonal': (E,), 'spherical': ()}[covariance_type]


def not_positive_definite():
    """The error of sklearn's _compute_precision_cholesky, which the reference's Gaussian log-pdf
    runs into (gaussian.py:26)."""
    return ValueError('Fitting the mixture model failed because some components have ill-defined '
                      'empirical covariance (not positive definite)')


# ---- weight_constant_axis -------------------------------------------------------------------
def constant_axes(weight_constant_axis, ndim):
    """int / list / tuple -> the set of negative axes of the (..., K, N) affiliation."""
    if isinstance(weight_constant_axis, int):
        weight_constant_axis = (weight_constant_axis,)
    return {a % ndim - ndim for a in weight_constant_axis}


def is_uniform(weight_constant_axis, ndim):
    """The class axis as an int: the only spelling the reference's estimate_mixture_weight maps
    to the constant 1 / K (mixture_model_utils.py:180-183)."""
    return isinstance(weight_constant_axis, int) and weight_constant_axis % ndim - ndim == -2


def fused_weight_mode(weight_constant_axis, ndim, ones=False):
    """The modes the single-launch kernels carry: (-1,) / -1 -> per-class weights, int -2 ->
    uniform 1 / K; None: weights that couple the independent problems (cooperative kernel or
    step-wise loop).  `ones` (GMM): tuple (-2,) -- the default of GMMTrainer.fit_predict -- takes
    the general path of estimate_mixture_weight, which averages over the class axis and
    L1-normalises along it, i.e. a (1, N) array of ones (:192-201) -> WEIGHT_ONES."""
    if is_uniform(weight_constant_axis, ndim):
        return _lib.WEIGHT_UNIFORM
    axes = constant_axes(weight_constant_axis, ndim)
    if axes == {-1}:
        return _lib.WEIGHT_PER_CLASS_MEAN
    if ones and axes == {-2}:
        return WEIGHT_ONES
    return None


def shared_weight_mode(weight_constant_axis, ndim):
    """weight_constant_axis that averages the weights over the last independent axis (the
    frequency bins): (-3,) and (-3, -1) run in the cooperative kernels."""
    axes = constant_axes(weight_constant_axis, ndim)
    if ndim >= 3 and axes == {-3}:
        return _lib.WEIGHT_SHARED_KT
    if ndim >= 3 and axes == {-3, -1}:
        return _lib.WEIGHT_SHARED_K
    return None


# ---- mixture weights ------------------------------------------------------------------------
def uniform_weight(K, device):
    """The constant (K, 1) array 1 / K of weight_constant_axis=-2 (mixture_model_utils.py:180-183)."""
    t = _lib.torch()
    return t.full((K, 1), 1.0 / K, dtype=t.float64, device=device)


def fused_weight(mode, weight, indep, K, device):
    """Reference-shaped weight of a single-launch fit: `weight` (B, K) from the kernel."""
    if mode == _lib.WEIGHT_UNIFORM:
        return uniform_weight(K, device)
    return weight.reshape(*indep, K, 1)


def _l1_normalize_where(x, axis, eps):
    """x / sum|x| along axis; a zero sum is replaced by eps
    (reference: distribution/utils.py:223-256 with ord=1, eps_style='where')."""
    s = np.sum(np.abs(x), axis=axis, keepdims=True)
    return x / np.where(s == 0, eps, s)


def host_estimate_mixture_weight(affiliation, saliency, weight_constant_axis):
    """The formula itself, for the axis sets pbbss_estimate_mixture_weight does not serve (a tuple
    that contains the class axis, a non-trailing block of independent axes, a saliency with more
    than 16 classes): a mean / normalised sum over a handful of axes, not on the hot path."""
    if saliency is None:
        return affiliation.mean(axis=weight_constant_axis, keepdims=True)
    weighted = (affiliation * saliency[..., None, :]).sum(
        axis=weight_constant_axis, keepdims=True)
    return _l1_normalize_where(weighted, axis=-2, eps=1e-10)


def kernel_weight(aff, sal, weight_constant_axis, indep):
    """estimate_mixture_weight (mixture_model_utils.py:133-203) on the device for the
    axis sets that occur in practice: the trailing `r` independent axes and / or the frame
    axis.  aff (*indep, K, N) device tensor, sal (*indep, N) or None.
    Returns the reference-shaped weight (keepdims) as a device tensor, or None if the axis
    set is not of that form (the caller then takes the host formula)."""
    nd = len(indep) + 2
    axes = sorted(a + nd for a in constant_axes(weight_constant_axis, nd))
    if nd - 2 in axes:  # the class axis: only the scalar form -2 is defined (handled earlier)
        return None
    red_n = (nd - 1) in axes
    ind_axes = [a for a in axes if a < nd - 2]
    r = len(ind_axes)
    if ind_axes != list(range(nd - 2 - r, nd - 2)):
        return None  # not a trailing block of independent axes
    K, N = aff.shape[-2:]
    Bi = int(np.prod(indep[len(indep) - r:], dtype=np.int64)) if r else 1
    Bo = int(np.prod(indep[:len(indep) - r], dtype=np.int64)) if len(indep) > r else 1
    a4 = aff.reshape(Bo, Bi, K, N).contiguous()
    s3 = None if sal is None else sal.reshape(Bo, Bi, N).contiguous()
    w = engine.estimate_mixture_weight(a4, s3, reduce_inner=r > 0, reduce_n=red_n)
    if w is None:  # not served (saliency with K > 16): the caller takes the host formula
        return None
    shape = list(indep[:len(indep) - r]) + [1] * r + [K, 1 if red_n else N]
    return w.reshape(shape)


def device_weight(aff, sal, weight_constant_axis, indep, on_host=None):
    """estimate_mixture_weight, reference-shaped (keepdims), as a device tensor: the constant
    1 / K, the reduction kernel, or -- for the axis sets the kernel does not cover (e.g. the
    class axis in a tuple) -- the NumPy formula (`on_host()` is called when that happens)."""
    t = _lib.torch()
    if is_uniform(weight_constant_axis, len(indep) + 2):
        return uniform_weight(aff.shape[-2], aff.device)
    w = kernel_weight(aff, sal, weight_constant_axis, indep)
    if w is None:
        if on_host is not None:
            on_host()
        w = _lib.to_device(host_estimate_mixture_weight(
            _lib.to_host(aff), None if sal is None else _lib.to_host(sal), weight_constant_axis),
            t.float64, device=aff.device)
    return w


# ---- independent axes -> one batch axis -----------------------------------------------------
def flatten_param(x, indep, tail_shape, dtype, device=None):
    """Model parameter (NumPy or torch) that broadcasts against (*indep, *tail_shape) ->
    contiguous (B, *tail_shape) device tensor of `dtype`."""
    x = _lib.to_device(x, dtype)
    if device is not None:
        x = x.to(device)
    return x.expand(*indep, *tail_shape).reshape(-1, *tail_shape).contiguous()


def flatten_weight(w, indep):
    """Reference-shaped (possibly lower-rank, keepdims) weight (..., K or 1, N or 1) device tensor
    -> (B or 1, K or 1, N or 1) for `engine.log_pdf_to_affiliation`: the independent axes are
    flattened, and they stay ONE singleton axis unless the array really varies there (the engine
    turns singleton axes into zero strides)."""
    while w.ndim < len(indep) + 2:
        w = w.unsqueeze(0)
    if any(a != 1 for a in w.shape[:-2]):
        w = w.expand(*indep, *w.shape[-2:])
    return w.reshape(-1, *w.shape[-2:]).contiguous()


# ---- the argument preamble of fit -----------------------------------------------------------
@dataclass
class FitArguments:
    y: object  # (*indep, N, D) device tensor
    indep: tuple
    N: int
    D: int
    K: int  # None when the initialisation is a model
    gamma0: object  # (*indep, K, N) float64 device tensor; None when the initialisation is a model
    saliency: object  # (B, N) float64 contiguous device tensor or None
    weight_constant_axis: object  # int or tuple
    like_torch: bool

    @property
    def ndim(self):
        return len(self.indep) + 2


def check_one_of(initialization, num_classes):
    assert xor(initialization is None, num_classes is None), (
        "Incompatible input combination. "
        "Exactly one of the two inputs has to be None: "
        f"{initialization is None} xor {num_classes is None}"
    )


def prepare_fit(y, initialization, num_classes, saliency, weight_constant_axis, *, complex_input,
                model_type=None):
    """What every `fit` does with its arguments before it looks at the model family: the
    reference's assertions, the observation on the device, the initial affiliations (random
    ones from the global NumPy RNG exactly as the reference) and the saliency per flattened
    problem.  `model_type` (CACGMM): the trainer also resumes from a fitted model of that type and
    checks an array initialisation as cacgmm.py:211-225 does (the other trainers hand whatever
    they are given to the device and broadcast it)."""
    check_one_of(initialization, num_classes)
    like_torch = _lib.is_torch(y)
    t = _lib.torch()
    y = _lib.to_device(y)
    if complex_input:
        if y.dtype not in (t.complex64, t.complex128):
            raise AssertionError(y.dtype)  # reference: assert np.iscomplexobj(y)
        assert y.shape[-1] > 1, y.shape
    else:
        assert not y.is_complex(), y.dtype
    *indep, N, D = y.shape
    indep = tuple(indep)
    if initialization is None:
        # global NumPy RNG, as the reference (utils.random_affiliation)
        gamma0 = random_affiliation((*indep, num_classes, N), y.device)
    elif model_type is not None and isinstance(initialization, model_type):
        gamma0 = num_classes = None
    else:
        if model_type is not None:
            if not (isinstance(initialization, np.ndarray) or _lib.is_torch(initialization)):
                raise TypeError('No sufficient initialization.')
            shape = (*indep, initialization.shape[-2], N)
            assert shape[-2] > 1, shape[-2]
            assert initialization.ndim == len(shape), (initialization.shape, shape)
            assert tuple(initialization.shape[-2:]) == shape[-2:], (initialization.shape, shape)
        gamma0 = _lib.to_device(initialization, t.float64).to(y.device)
        num_classes = gamma0.shape[-2]
        gamma0 = gamma0.expand(*indep, num_classes, N)
    if isinstance(weight_constant_axis, list):
        weight_constant_axis = tuple(weight_constant_axis)
    sal = None
    if saliency is not None:
        sal = flatten_param(saliency, indep, (N,), t.float64, y.device)
    return FitArguments(y=y, indep=indep, N=N, D=D, K=num_classes, gamma0=gamma0, saliency=sal,
                        weight_constant_axis=weight_constant_axis, like_torch=like_torch)


def check_dimension(trainer, D):
    """cwmm.py / cbmm.py: a trainer is bound to the dimension of its first fit."""
    if trainer.dimension is None:
        trainer.dimension = D
    else:
        assert trainer.dimension == D, (
            'You initialized the trainer with a different dimension than '
            'you are using to fit a model. Use a new trainer, when you '
            'change the dimension.')


# ---- between E- and M-step ------------------------------------------------------------------
def apply_inline_permutation_alignment(affiliation, *, quadratic_form=None,
                                       weight_constant_axis, aligner, status_out=None):
    """Run a permutation-alignment solver between E- and M-step.

    Reference: mixture_model_utils.py:264-306.  affiliation / quadratic_form
    are (F, K, T); `aligner` is any object with
    calculate_mapping((K, F, T)) -> (K, F) and apply_mapping(x, mapping)
    (e.g. pb_bss.permutation_alignment.DHTVPermutationAlignment).

    `status_out` (a list; not in the reference) opts a device caller into the asynchronous
    route: with device tensors and an aligner that offers `calculate_mapping_async` the
    solver's status words are appended to the list instead of being read back here, and the
    caller checks them when it next synchronises.
    """
    msg = ('Inline permutation alignment needs affiliation.ndim == 3 '
           f'({affiliation.shape}) and a frequency-constant mixture weight '
           f'(weight_constant_axis={weight_constant_axis}).')
    assert affiliation.ndim == 3, msg
    assert weight_constant_axis in ((-3,), (-3, -1), -3), msg
    def swap(x):  # (F, K, T) <-> (K, F, T) for NumPy arrays and torch tensors alike
        return x.permute(1, 0, 2).contiguous() if hasattr(x, 'permute') else x.transpose(1, 0, 2)

    if status_out is not None and hasattr(affiliation, 'permute') and affiliation.is_cuda \
            and hasattr(aligner, 'calculate_mapping_async'):
        # device loop (CACGMMTrainer._fit_stepwise): no host synchronisation per EM iteration --
        # the status words are queued for the caller -- and the reverse mapping is applied as a
        # gather along the class axis of the (F, K, T) arrays themselves, without the two
        # transposed copies per array of the generic route below
        t = _lib.torch()
        F, K, T = affiliation.shape
        mapping, st = aligner.calculate_mapping_async(
            affiliation.to(t.float64).permute(1, 0, 2).contiguous()[None])
        status_out.append(st)
        idx = mapping[0].t().to(t.int64)[:, :, None].expand(F, K, T)
        aligned = affiliation.gather(1, idx)
        if quadratic_form is None:
            return aligned
        return aligned, quadratic_form.gather(1, idx)
    kft = swap(affiliation)
    mapping = aligner.calculate_mapping(kft)
    aligned = swap(aligner.apply_mapping(kft, mapping))
    if quadratic_form is None:
        return aligned
    q = aligner.apply_mapping(swap(quadratic_form), mapping)
    return aligned, swap(q)


def is_device_aligner(aligner):
    """The project's own solvers take device tensors; anything else is a foreign (NumPy) object."""
    return type(aligner).__module__.startswith('pb_bss_amd')


def align(aligner, aff, weight_constant_axis, quadratic_form=None, status_out=None):
    """`apply_inline_permutation_alignment` on device tensors (F, K, T) -> device tensors, for
    either kind of aligner.  `status_out`: see there (device aligners only)."""
    if is_device_aligner(aligner):
        return apply_inline_permutation_alignment(
            affiliation=aff, quadratic_form=quadratic_form,
            weight_constant_axis=weight_constant_axis, aligner=aligner, status_out=status_out)
    # a foreign (NumPy) aligner object: the one host excursion left
    t = _lib.torch()
    out = apply_inline_permutation_alignment(
        affiliation=_lib.to_host(aff),
        quadratic_form=None if quadratic_form is None else _lib.to_host(quadratic_form),
        weight_constant_axis=weight_constant_axis, aligner=aligner)
    if quadratic_form is None:
        return _lib.to_device(out, t.float64, device=aff.device)
    return tuple(_lib.to_device(x, t.float64, device=aff.device) for x in out)


# ---- the step-wise EM loop ------------------------------------------------------------------
def stepwise_em(gamma0, iterations, log_pdf, m_step, *, saliency, weight_constant_axis,
                aligner=None, affiliation_eps=0.):
    """The reference's loop statement by statement (cwmm.py:151-182, cbmm.py:181-203,
    vmfmm.py:131-172, gmm.py:121-171) for the options the fused kernels do not carry --
    weights shared over independent axes or frame-varying, an inline aligner, a clipped softmax:

        affiliation = predict(model)                -> log_pdf(model) + pbbss_log_pdf_to_affiliation
        affiliation = aligner(affiliation)          (optional)
        weight      = estimate_mixture_weight(...)  -> pbbss_estimate_mixture_weight
        model       = Trainer()._fit(y, affiliation * saliency)   -> m_step(...)

    gamma0 (*indep, K, N) float64 device tensor; saliency (B, N) device tensor (as prepare_fit
    returns it) or None (None: the weight is a mean, otherwise an L1-normalised sum -- an all-ones
    saliency is not the same thing); log_pdf(model) -> class log-pdfs (B, K, N); m_step(masked (B, K, N)
    contiguous) -> model.  Nothing returns to the host inside the loop, except for a foreign
    (NumPy) aligner object.  -> (model, reference-shaped weight)."""
    shape = tuple(gamma0.shape)
    indep, (K, N) = shape[:-2], shape[-2:]
    aff = gamma0.contiguous()
    if saliency is not None:
        saliency = saliency.reshape(*indep, N)
    model = weight = None
    for _ in range(iterations):
        if model is not None:
            aff = engine.log_pdf_to_affiliation(
                log_pdf(model), flatten_weight(weight, indep),
                affiliation_eps=affiliation_eps).reshape(shape)
            if aligner is not None:
                aff = align(aligner, aff, weight_constant_axis).contiguous()
        weight = device_weight(aff, saliency, weight_constant_axis, indep)
        masked = aff if saliency is None else aff * saliency[..., None, :]
        model = m_step(masked.reshape(-1, K, N).contiguous())
    return model, weight
