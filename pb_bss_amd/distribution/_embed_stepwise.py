"""Step-wise EM loop of the real-embedding mixtures (VMFMM, GMM) on the device, for the options
the fused loops (`pbbss_vmfmm_fit`, `pbbss_gmm_fit`, `pbbss_gmm_full_fit`) do not carry:
`weight_constant_axis` sets beyond (-1,) / -2 -- weights shared over independent axes,
frame-varying weights -- and `covariance_type='diagonal'`.

It is the reference's loop statement by statement (vmfmm.py:131-172, gmm.py:121-171):

    affiliation = predict(model)                  -> class log-pdfs + log_pdf_to_affiliation
    weight      = estimate_mixture_weight(...)    -> pbbss_estimate_mixture_weight
    component   = Trainer()._fit(y, affiliation * saliency)

with every step a device kernel (`pbbss_embed_log_pdf` / `pbbss_gauss_full_log_pdf`,
`pbbss_log_pdf_to_affiliation`, `pbbss_estimate_mixture_weight`, `pbbss_embed_fit` /
`pbbss_gauss_full_fit`); nothing returns to the host inside the loop.
"""
from .. import _lib, engine
from . import _mixture as mix

KINDS = {'vmf': _lib.EMBED_VMF, 'spherical': _lib.EMBED_GAUSS_SPHERICAL,
         'diagonal': _lib.EMBED_GAUSS_DIAG, 'full': _lib.EMBED_GAUSS_FULL}


def log_pdf(kind, yb, mean, scale):
    """Class log-pdfs (B, K, N) of the components (mean (B,K,E), scale by kind)."""
    if kind == 'full':
        lp, st = engine.gauss_full_log_pdf(yb, mean, scale)
        if int(st.item()) != 0:
            raise mix.not_positive_definite()
        return lp
    if kind == 'diagonal':
        # the reference's DiagonalGaussian.log_pdf takes the (K, E) precisions of ONE mixture as a
        # K x E matrix shared by its classes (gaussian.py:87-91): one call per independent mixture
        return _lib.torch().cat([engine.embed_log_pdf(yb[b:b + 1], KINDS[kind], mean[b:b + 1],
                                                      scale[b:b + 1]) for b in range(yb.shape[0])])
    return engine.embed_log_pdf(yb, KINDS[kind], mean, scale)


def affiliation(kind, yb, mean, scale, weight, indep):
    """predict(): softmax of the class log-pdfs with a reference-shaped weight array."""
    return engine.log_pdf_to_affiliation(log_pdf(kind, yb, mean, scale),
                                         mix.flatten_weight(weight, indep))


def fit(kind, y, gamma0, iterations, saliency, weight_constant_axis, *, fixed_scale=None,
        min_concentration=1e-10, max_concentration=500.):
    """y (*indep, N, E) device tensor, gamma0 (*indep, K, N) float64 device tensor, saliency
    (B, N) device tensor or None.
    -> dict(mean (*indep,K,E), scale, weight (reference shape)) of device tensors."""
    N, E = y.shape[-2:]
    yb = y.reshape(-1, N, E)

    def m_step(wts):
        if kind == 'full':
            mean, scale = engine.gauss_full_fit(yb, wts)
        else:
            mean, scale = engine.embed_fit(yb, KINDS[kind], wts, normalize=(kind == 'vmf'),
                                           min_concentration=min_concentration,
                                           max_concentration=max_concentration)
        if fixed_scale is not None:
            scale = fixed_scale.reshape(scale.shape)
        return mean, scale

    (mean, scale), weight = mix.stepwise_em(
        gamma0, iterations, lambda model: log_pdf(kind, yb, *model), m_step,
        saliency=saliency, weight_constant_axis=weight_constant_axis)
    return dict(mean=mean, scale=scale, weight=weight)
