"""STFT edge of the separation path: audio -> STFT -> (mixture model, beamformer) -> audio
without leaving the device, and the gammatone filterbank of the
reference's transform/gammatone.py."""
from .gammatone import gammatone_filterbank, calculate_cfs, Hz_2_ERBS, ERBS_2_Hz
from .stft import stft, istft, stft_frames_to_samples, biorthogonal_window, analysis_window

__all__ = ['stft', 'istft', 'stft_frames_to_samples', 'biorthogonal_window', 'analysis_window',
           'gammatone_filterbank', 'calculate_cfs', 'Hz_2_ERBS', 'ERBS_2_Hz']
