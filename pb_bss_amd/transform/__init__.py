"""STFT edge of the separation path: audio -> STFT -> (mixture model, beamformer) -> audio
without leaving the device, and the gammatone filterbank of the
reference's transform/gammatone.py, and the phase reconstruction (Griffin-Lim, MISI) of its
transform/griffin_lim_module.py, and WPE dereverberation with the signatures of nara_wpe.wpe (the
stage in front of the mixture model), offline and frame-recursive, and the streaming STFT / inverse
STFT that feed and drain the frame-recursive stages block by block."""
from .gammatone import gammatone_filterbank, calculate_cfs, Hz_2_ERBS, ERBS_2_Hz
from .stft import stft, istft, stft_frames_to_samples, biorthogonal_window, analysis_window
from .griffin_lim_module import GriffinLim, MISI
from .wpe import (wpe, get_power, get_power_inverse, get_correlations, get_filter_matrix,
                  perform_filter_operation, recursive_wpe, online_wpe_step, OnlineWPE,
                  OnlineWPEState)
from .stft_online import OnlineSTFT, OnlineISTFT, OnlineSTFTState, OnlineISTFTState

__all__ = ['stft', 'istft', 'stft_frames_to_samples', 'biorthogonal_window', 'analysis_window',
           'gammatone_filterbank', 'calculate_cfs', 'Hz_2_ERBS', 'ERBS_2_Hz', 'GriffinLim', 'MISI',
           'wpe', 'get_power', 'get_power_inverse', 'get_correlations', 'get_filter_matrix',
           'perform_filter_operation', 'recursive_wpe', 'online_wpe_step', 'OnlineWPE',
           'OnlineWPEState', 'OnlineSTFT', 'OnlineISTFT', 'OnlineSTFTState', 'OnlineISTFTState']
