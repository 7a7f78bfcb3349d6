"""Drop-in for the hot-path part of pb_bss.distribution
(reference: pb_bss/distribution/__init__.py)."""
from .complex_angular_central_gaussian import (
    ComplexAngularCentralGaussian,
    ComplexAngularCentralGaussianTrainer,
    normalize_observation,
    sample_complex_angular_central_gaussian,
)
from .complex_circular_symmetric_gaussian import (
    ComplexCircularSymmetricGaussian,
    ComplexCircularSymmetricGaussianTrainer,
)
from .cacgmm import CACGMM, CACGMMTrainer, sample_cacgmm
from .complex_watson import ComplexWatson, ComplexWatsonTrainer
from .cwmm import CWMM, CWMMTrainer
from .complex_bingham import ComplexBingham, ComplexBinghamTrainer
from .cbmm import CBMM, CBMMTrainer
from .von_mises_fisher import VonMisesFisher, VonMisesFisherTrainer
from .vmfmm import VMFMM, VMFMMTrainer
from .gaussian import DiagonalGaussian, Gaussian, SphericalGaussian, GaussianTrainer
from .gmm import GMM, GMMTrainer, BinaryGMM, BinaryGMMTrainer
from .gcacgmm import GCACGMM, GCACGMMTrainer
from .vmfcacgmm import VMFCACGMM, VMFCACGMMTrainer
from .online_cacgmm import OnlineCACGMM, OnlineCACGMMState, recursive_cacgmm

__all__ = [
    'CACGMM', 'CACGMMTrainer', 'CWMM', 'CWMMTrainer', 'CBMM', 'CBMMTrainer',
    'ComplexBingham', 'ComplexBinghamTrainer',
    'VonMisesFisher', 'VonMisesFisherTrainer', 'VMFMM', 'VMFMMTrainer',
    'Gaussian', 'DiagonalGaussian', 'SphericalGaussian', 'GaussianTrainer', 'GMM', 'GMMTrainer',
    'BinaryGMM', 'BinaryGMMTrainer', 'GCACGMM', 'GCACGMMTrainer',
    'VMFCACGMM', 'VMFCACGMMTrainer',
    'ComplexWatson', 'ComplexWatsonTrainer',
    'ComplexAngularCentralGaussian', 'ComplexAngularCentralGaussianTrainer',
    'ComplexCircularSymmetricGaussian', 'ComplexCircularSymmetricGaussianTrainer',
    'normalize_observation', 'sample_cacgmm', 'sample_complex_angular_central_gaussian',
    'recursive_cacgmm', 'OnlineCACGMM', 'OnlineCACGMMState',
]
