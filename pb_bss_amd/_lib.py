"""ctypes binding of libpbbss_hip.so (the C ABI declared in include/pbbss.h).

The product path has NO CPU fallback: if the shared library is missing or a
call fails this module raises.  PyTorch-ROCm is used only as the owner of
device memory and streams; all arithmetic happens inside the HIP library.

The calling convention of the header lives here, once: SIGNATURES describes every export as
data, `launch` (handle first, stream last) and `control` (handle, no stream) marshal a call from
it.  The modules of the package name the export and hand over tensors and numbers; only the few
host functions without a handle are called on `load()` directly.
"""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get('PBBSS_LIB', 'libpbbss_hip.so'))

# ---- constants mirrored from include/pbbss.h ---------------------------------
OK = 0
ERR_INVALID_ARG = -1
ERR_UNSUPPORTED = -2
ERR_HIP = -3
ERR_LDS_CAPACITY = -4
ERR_INTERNAL = -5

ST_NONFINITE = 1
ST_EIG_NOCONV = 2
ST_FLOORED = 4
ST_SLOWPATH = 8
ST_NOT_POSDEF = 16
ST_SINGULAR = 32
ST_SOLVE_NOCONV = 64  # complex Bingham parameter solve did not converge
ST_ZERO_SIGNAL = 128  # BSS-Eval: an all-zero reference or estimate

COVNORM = {False: 0, None: 0, 'eigenvalue': 1, 'trace': 2}
WEIGHT_PER_CLASS_MEAN = 0
WEIGHT_UNIFORM = 1
WEIGHT_SHARED_K = 2   # weight_constant_axis=(-3, -1), pbbss_cacgmm_fit_shared only
WEIGHT_SHARED_KT = 3  # weight_constant_axis=(-3,)
LAYOUT_TD = 0
LAYOUT_DT = 1

EMBED_VMF = 0
EMBED_GAUSS_SPHERICAL = 1
EMBED_GAUSS_FULL = 2
EMBED_GAUSS_DIAG = 3
# weight_constant_axis of the joint models -> PBBSS_JOINT_WEIGHT_*
JOINT_WEIGHT_FK, JOINT_WEIGHT_UNIFORM, JOINT_WEIGHT_K, JOINT_WEIGHT_KT, JOINT_WEIGHT_CONST = range(5)


class EmOpts(ctypes.Structure):
    """struct pbbss_em_opts"""
    _fields_ = [
        ('iterations', ctypes.c_int32),
        ('covariance_norm', ctypes.c_int32),
        ('weight_mode', ctypes.c_int32),
        ('hermitize', ctypes.c_int32),
        ('layout', ctypes.c_int32),
        ('y_is_c128', ctypes.c_int32),
        ('final_predict', ctypes.c_int32),
        ('force_eig', ctypes.c_int32),
        ('affiliation_eps', ctypes.c_double),
        ('eigenvalue_floor', ctypes.c_double),
        ('precision', ctypes.c_int32),
        ('reserved', ctypes.c_int32),
    ]


PRECISION = {'f64': 0, 'float64': 0, None: 0, 'f32': 1, 'float32': 1}


class CwmmOpts(ctypes.Structure):
    """struct pbbss_cwmm_opts"""
    _fields_ = [
        ('iterations', ctypes.c_int32),
        ('weight_mode', ctypes.c_int32),
        ('y_is_c128', ctypes.c_int32),
        ('final_predict', ctypes.c_int32),
        ('n_coef', ctypes.c_int32),
        ('group', ctypes.c_int32),
        ('ev_min', ctypes.c_double),
        ('ev_max', ctypes.c_double),
        ('max_concentration', ctypes.c_double),
    ]


class CbmmOpts(ctypes.Structure):
    """struct pbbss_cbmm_opts"""
    _fields_ = [
        ('iterations', ctypes.c_int32),
        ('weight_mode', ctypes.c_int32),
        ('y_is_c128', ctypes.c_int32),
        ('final_predict', ctypes.c_int32),
        ('max_concentration', ctypes.c_double),
        ('eigenvalue_eps', ctypes.c_double),
        ('norm_eps', ctypes.c_double),
    ]


class MixOpts(ctypes.Structure):
    """struct pbbss_mix_opts"""
    _fields_ = [
        ('iterations', ctypes.c_int32),
        ('kind', ctypes.c_int32),
        ('weight_mode', ctypes.c_int32),
        ('embedding_is_f64', ctypes.c_int32),
        ('obs_is_c128', ctypes.c_int32),
        ('final_predict', ctypes.c_int32),
        ('inline_pa', ctypes.c_int32),
        ('covariance_norm', ctypes.c_int32),
        ('min_concentration', ctypes.c_double),
        ('max_concentration', ctypes.c_double),
        ('affiliation_eps', ctypes.c_double),
        ('eigenvalue_floor', ctypes.c_double),
        ('spatial_weight', ctypes.c_double),
        ('spectral_weight', ctypes.c_double),
        ('sharded', ctypes.c_int32),
        ('reserved', ctypes.c_int32),
    ]


MASK_IBM, MASK_WIENER, MASK_IRM, MASK_IAM, MASK_PSM, MASK_ICM, MASK_BIASED = range(7)
MASK_ST_NO_THRESHOLD = 1
EVAL_F32, EVAL_F64, EVAL_C64, EVAL_C128 = range(4)


class MaskGeom(ctypes.Structure):
    """struct pbbss_mask_geom"""
    _fields_ = [
        ('size', ctypes.c_int64 * 4),
        ('x_stride', ctypes.c_int64 * 4),
        ('out_stride', ctypes.c_int64 * 4),
        ('x_source_stride', ctypes.c_int64),
        ('x_sensor_stride', ctypes.c_int64),
        ('out_source_stride', ctypes.c_int64),
        ('out_target_stride', ctypes.c_int64),
        ('sources', ctypes.c_int32),
        ('sensors', ctypes.c_int32),
    ]


# ---- the C ABI as data: argument types of every export of include/pbbss.h ---------------
# (tests/test_capi_symbols.py compares the kind of every parameter with the header's prototypes)
vp, i32, u32, i64, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_int64, ctypes.c_double
P = ctypes.POINTER
vpp, i32p, i64p, f32p = P(vp), P(i32), P(i64), P(ctypes.c_float)
SIGNATURES = {
    'pbbss_version': [],
    'pbbss_error_string': [i32],
    'pbbss_create': [vpp, i32],
    'pbbss_destroy': [vp],
    'pbbss_normalize_observation': [vp, vp, i32, i64, i32, i32, vp, vp],
    'pbbss_cacgmm_fit': [vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, P(EmOpts), vp, vp, vp,
        vp, vp, vp, vp],
    'pbbss_cacgmm_fit_shared': [vp, vp, i64, i32, i32, i32, i64, vp, vp, vp, vp, vp, vp, P(EmOpts),
        vp, vp, vp, vp, vp, vp, vp],
    'pbbss_cacgmm_predict': [vp, vp, i64, i32, i32, i32, vp, vp, vp, i64, i64, i64, vp, i32, i32,
        dbl, vp, vp, vp, vp],
    'pbbss_cacg_m_step': [vp, vp, i64, i32, i32, i32, vp, vp, i32, i32, i32, dbl, vp, vp, vp, vp,
        vp],
    'pbbss_heev_batched': [vp, vp, i64, i32, vp, vp, vp, vp],
    'pbbss_psd': [vp, vp, i32, i64, i32, i32, i32, vp, i32, vp, vp],
    'pbbss_gev': [vp, vp, vp, i64, i32, vp, vp, vp],
    'pbbss_gev_general': [vp, vp, vp, i64, i32, vp, vp, vp, vp],
    'pbbss_comm_unique_id': [vp],
    'pbbss_comm_create': [vp, vp, i32, i32],
    'pbbss_comm_destroy': [vp],
    'pbbss_comm_info': [vp, i32p, i32p],
    'pbbss_shard_bounds': [i64, i32, i32, i64p, i64p],
    'pbbss_allgather_masks': [vp, vp, i32, i64, i64, i64, vp, vp],
    'pbbss_allgather_unpack': [vp, vp, i32, i32, i64, i64, i64, vp, vp],
    'pbbss_estimate_mixture_weight': [vp, vp, vp, i64, i64, i32, i64, i32, i32, vp, vp],
    'pbbss_log_pdf_to_affiliation': [vp, vp, i64, i32, i64, vp, i64, i64, i64, vp, dbl, vp, vp],
    'pbbss_log_pdf_to_affiliation_inline_pa': [vp, vp, vp, i64, i32, i64, vp, i64, i64, i64, vp,
        dbl, vp, vp, vp],
    'pbbss_solve': [vp, vp, vp, i64, i32, i32, vp, vp, vp],
    'pbbss_mvdr_souden': [vp, vp, vp, i64, i32, dbl, vp, vp, vp, vp, vp],
    'pbbss_mvdr': [vp, vp, vp, i64, i32, vp, vp, vp],
    'pbbss_ban': [vp, vp, vp, i64, i32, vp, vp],
    'pbbss_apply_beamforming_vector': [vp, vp, vp, i32, i64, i32, i32, vp, vp],
    'pbbss_apply_beamforming_vector_shared': [vp, vp, vp, i32, i64, i64, i32, i32, vp, vp],
    'pbbss_select_reference_channel': [vp, vp, vp, vp, i64, i64, i32, i64, i64, dbl, vp, vp, vp,
        vp],
    'pbbss_set_timing': [vp, i32],
    'pbbss_last_kernel_ms': [vp, f32p],
    'pbbss_kernel_ms_lagged': [vp, i32, f32p],
    'pbbss_set_phase_profile': [vp, vp],
    'pbbss_dhtv_calculate_mapping': [vp, vp, i64, i32, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp],
    'pbbss_apply_mapping': [vp, vp, vp, i64, i32, i32, i32, vp, vp],
    'pbbss_cwmm_fit': [vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, P(CwmmOpts), vp, vp, vp, vp,
        vp, vp, vp, vp, vp],
    'pbbss_cbmm_fit': [vp, vp, i64, i32, i32, i32] + [vp] * 5 + [P(CbmmOpts)] + [vp] * 8,
    'pbbss_cbingham_find_eigenvalues': [vp, vp, i64, i32, dbl, dbl, vp, vp, vp],
    'pbbss_wmwf': [vp, vp, vp, i64, i32, dbl, i32, vp, vp, vp, vp, vp],
    'pbbss_set_split_tail': [vp, i32],
    'pbbss_split_error': [vp, i32p],
    'pbbss_split_reset': [vp],
    'pbbss_set_spin_limit': [vp, u32],
    'pbbss_embed_log_pdf': [vp, vp, i32, i64, i64, i32, i32, i32, vp, vp, vp, vp],
    'pbbss_embed_fit': [vp, vp, i32, i64, i64, i32, i32, i32, i32, vp, dbl, dbl, vp, vp, vp],
    'pbbss_vmfmm_fit': [vp, vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, P(MixOpts), vp, vp, vp, vp,
        vp, vp],
    'pbbss_joint_fit': [vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, P(MixOpts),
        vp, vp, vp, vp, vp, vp, vp, vp],
    'pbbss_lcmv': [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp],
    'pbbss_phase_correction': [vp, vp, i64, i64, i32, i32, i32, vp, vp, vp],
    'pbbss_snr_postfilter': [vp, vp, vp, vp, i64, i32, vp, vp],
    'pbbss_reference_channel_terms': [vp, vp, vp, vp, i64, i32, vp, vp, vp],
    'pbbss_rank_one_approximation': [vp, vp, vp, i64, i32, vp, vp],
    'pbbss_matvec': [vp, vp, vp, i64, i32, vp, vp],
    'pbbss_distortionless_normalization': [vp, vp, vp, vp, i64, i32, vp, vp],
    'pbbss_zero_degree_normalization': [vp, vp, i64, i32, i32, vp, vp],
    'pbbss_condition_covariance': [vp, vp, i64, i32, dbl, vp, vp],
    'pbbss_apply_online_beamforming_vector': [vp, vp, vp, i32, i64, i32, i32, vp, vp],
    'pbbss_set_dhtv_team': [vp, i32],
    'pbbss_set_dhtv_probe': [vp, i32],
    'pbbss_stft_num_frames': [i64, i32, i32, i32, i32, i32],
    'pbbss_stft': [vp, vp, i32, i64, i64, i32, i32, i32, vp, i32, i32, i32, i32, vp, vp],
    'pbbss_istft': [vp, vp, i32, i64, i32, i32, i32, i32, vp, i32, vp, i64, vp],
    'pbbss_griffin_lim': [vp, vp, i32, vp, i64, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp,
        i64, vp],
    'pbbss_pa_pairwise_mapping': [vp, vp, vp, i64, i32, i64, i32, vp, vp, i32, i32, vp, vp, i64,
        i64, vp, vp],
    'pbbss_pa_compose_mapping': [vp, vp, i64, i32, i64, vp],
    'pbbss_pa_mapping_from_scores': [vp, vp, i64, i32, i32, vp, vp, vp],
    'pbbss_gmm_fit': [vp, vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, P(MixOpts), vp, vp, vp,
        vp, vp, vp],
    'pbbss_gauss_full_fit': [vp, vp, i32, i64, i64, i32, i32, vp, vp, vp, vp],
    'pbbss_gauss_full_log_pdf': [vp, vp, i32, i64, i64, i32, i32, vp, vp, vp, vp, vp],
    'pbbss_gmm_full_fit': [vp, vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, P(MixOpts), vp, vp,
        vp, vp, vp, vp, vp],
    'pbbss_deflation_seed': [vp, vp, i32, i64, i32, i32, i32, i32, vp, i32, i32, dbl, i32, i32, i32,
        vp, vp, vp, vp],
    'pbbss_mask_pointwise': [vp, vp, i32, i32, P(MaskGeom), dbl, vp, i64, vp, vp],
    'pbbss_mask_lorenz': [vp, vp, i32, P(MaskGeom), dbl, dbl, dbl, vp, i32, vp, vp],
    'pbbss_mask_quantile': [vp, vp, i32, P(MaskGeom), i32, i64p, P(dbl), i32p, dbl, dbl, vp, i32,
        vp, vp],
    'pbbss_signal_power': [vp, vp, i32, i64, i64, i64, vp, vp],
    'pbbss_si_sdr': [vp, vp, vp, i32, i64, i32, i32, i64, i64, i64, i64, i64, vp, vp],
    'pbbss_output_sxr': [vp, vp, vp, i32, i64, i32, i32, i64, i32, vp, vp, vp, vp],
    'pbbss_input_sxr': [vp, vp, vp, i32, i64, i32, i32, i64, i32, i32, vp, vp],
    'pbbss_bss_eval_workspace': [i64, i32, i32, i64, i64, i32, i64p],
    'pbbss_bss_eval': [vp, vp, vp, i32, i64, i32, i32, i64, i64, i64, i64, i64, i32, i32, vp, vp,
        vp, vp, vp, vp, vp],
    'pbbss_bss_eval_system': [vp, vp, vp, i32, i64, i32, i32, i64, i64, i64, i64, i64, i32, vp, vp,
        vp],
    'pbbss_bss_eval_filters': [vp, vp, vp, i32, i64, i32, i32, i64, i64, i64, i64, i64, i32, i32,
        vp, vp, vp, vp, vp, vp, vp, vp, vp],
    'pbbss_bss_eval_phase_ms': [vp, f32p],
    'pbbss_kmeans_fit': [vp, vp, i32, i64, i64, i32, i32, vp, vp, i32, dbl, i32, vp, vp, vp, vp,
        vp],
    'pbbss_kmeans_predict': [vp, vp, i32, i64, i64, i32, i32, vp, vp, vp, vp, vp],
    'pbbss_kmeans_plusplus': [vp, vp, i32, i64, i64, i32, i32, vp, i32, vp, vp, vp, vp],
    'pbbss_srmr_vad': [vp, vp, i32, i64, i64, i32, vp, vp, vp],
    'pbbss_gammatone': [vp, vp, i32, i64, i64, vp, i32, vp, vp, vp],
    'pbbss_srmr_energies': [vp, vp, i64, i64, vp, i32, i32, vp, vp, vp],
    'pbbss_srmr_score': [vp, vp, i64, i32, vp, vp, vp, vp],
    'pbbss_resample_poly': [vp, vp, i32, i64, i64, i32, i32, vp, i32, vp, vp],
    'pbbss_stoi': [vp, vp, vp, i64, i64, i64, i64, i64, i64, i64, vp, vp, vp],
    'pbbss_ccsg_fit': [vp, vp, i32, i64, i64, i32, i32, vp, i32, dbl, vp, vp],
    'pbbss_ccsg_log_pdf': [vp, vp, i32, i64, i64, i32, i32, vp, vp, vp, vp, vp],
    'pbbss_wpe': [vp, vp, i32, i64, i32, i64, i64, i64, i64, i32, i32, i32, i64, i32, vp, vp, vp],
    'pbbss_wpe_power_inverse': [vp, vp, i32, i64, i32, i64, i64, i64, i64, i64, vp, vp, vp],
    'pbbss_wpe_correlations': [vp, vp, i32, i64, i32, i64, i64, i64, i64, vp, i32, i32, i32, vp,
        vp, vp],
    'pbbss_wpe_filter_matrix': [vp, vp, vp, i64, i32, i32, vp, vp, vp],
    'pbbss_wpe_apply_filter': [vp, vp, i32, i64, i32, i64, i64, i64, i64, vp, i32, i32, vp, vp],
    'pbbss_wpe_online': [vp, vp, i32, i64, i32, i64, i64, i64, i64, i32, i32, dbl, vp, vp, vp, vp,
        vp, vp, vp, vp],
    'pbbss_online_mvdr': [vp, vp, i32, i64, i32, i64, i64, i64, i64, vp, vp, i32, dbl, i32, vp, vp,
        vp, vp, vp, vp, vp],
    'pbbss_online_cacgmm': [vp, vp, i32, i64, i32, i32, i64, i64, i64, i64, dbl, dbl, i32, vp, vp,
        vp, vp, vp, vp, vp, vp, vp],
}
EXPORTS = tuple(SIGNATURES)
# include/pbbss_stream.h, the section of the ABI whose state lives in tensors of the caller: the
# handle only names the device, nothing of its memory is used (tests/test_stream_symbols.py);
# reached through launch_stream below
STREAM_SIGNATURES = {
    'pbbss_stft_stream': [vp, vp, i32, i64, i64, vp, vp, i64, i64, i32, i32, i32, i32, i32, vp,
        i32, i32, i32, vp, vp],
    'pbbss_istft_stream': [vp, vp, i32, i64, i32, i64, i64, i64, i32, i32, i32, vp, vp, i32, vp,
        i64, vp],
}


class PbbssError(RuntimeError):
    pass


_lib = None
_lib_lock = threading.Lock()


def load():
    """dlopen the HIP library; raises if it has not been built."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise PbbssError(
                f'{LIB_PATH} not found: build it with '
                '`make -C pb_bss_amd/csrc -j8` (or __graft_entry__.build()). '
                'There is no CPU fallback.')
        # PyTorch ships its own copy of the HIP runtime (torch/lib/libamdhip64.so).  It must be
        # mapped BEFORE this library is: the loader then resolves our libamdhip64.so.7 dependency
        # to that same copy.  Loaded the other way round, the process ends up with two HIP/HSA
        # runtimes and whichever initialises second reports "no ROCm-capable device".
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        for name, argtypes in {**SIGNATURES, **STREAM_SIGNATURES}.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = ctypes.c_char_p if name == 'pbbss_error_string' else ctypes.c_int
        _lib = lib
        return lib


def check(rc, what=''):
    if rc != OK:
        msg = load().pbbss_error_string(rc).decode()
        if rc == ERR_UNSUPPORTED:
            raise NotImplementedError(f'{what}: {msg}')
        raise PbbssError(f'{what}: {msg} (code {rc})')


# ---- device handles -----------------------------------------------------------
_handles = {}
_handles_lock = threading.Lock()


def torch():
    import torch as _torch
    return _torch


def require_gpu():
    t = torch()
    if not t.cuda.is_available():
        raise PbbssError(
            'pb_bss_amd needs a ROCm GPU (torch.cuda.is_available() is False); '
            'there is no CPU fallback in the product path.')
    return t


def handle(device_index=None):
    """One C handle per (device, host thread)."""
    if device_index is not None:  # the per-call path: no GPU query, no lock once it exists
        h = _handles.get((device_index, threading.get_ident()))
        if h is not None:
            return h
    t = require_gpu()
    if device_index is None:
        device_index = t.cuda.current_device()
    key = (device_index, threading.get_ident())
    with _handles_lock:
        h = _handles.get(key)
        if h is None:
            lib = load()
            hp = ctypes.c_void_p()
            check(lib.pbbss_create(ctypes.byref(hp), device_index), 'pbbss_create')
            h = hp
            _handles[key] = h
        return h


def current_stream(device_index=None):
    return torch().cuda.current_stream(device_index)


def is_capturing():
    return torch().cuda.is_current_stream_capturing()


def stream_ptr(device_index=None, stream=None):
    """hipStream_t of `stream`, by default of the current torch stream of the device"""
    if stream is None:
        stream = current_stream(device_index)
    return ctypes.c_void_p(stream.cuda_stream)


_CTYPES_POINTERS = (ctypes._SimpleCData, ctypes.Array, bytes)  # c_void_p, arrays, string buffers


def ptr(tensor):
    """Device pointer of a contiguous torch tensor (None -> NULL); what already is a ctypes
    pointer argument passes through."""
    if tensor is None or isinstance(tensor, _CTYPES_POINTERS):
        return tensor
    assert tensor.is_cuda and tensor.is_contiguous(), (tensor.device, tensor.stride())
    return ctypes.c_void_p(tensor.data_ptr())


def view_ptr(tensor):
    """Device pointer of a (possibly strided) view; the strides travel separately."""
    assert tensor.is_cuda, tensor.device
    return ctypes.c_void_p(tensor.data_ptr())


# ---- the calling convention ---------------------------------------------------------------------
def _ref(a):
    """POINTER(T) slot: a Structure or a scalar ctypes object goes by reference, an array as it
    is."""
    return ctypes.byref(a) if isinstance(a, (ctypes.Structure, ctypes._SimpleCData)) else a


# export -> one converter per parameter behind the handle (the stream's included where there is
# one): pure data from SIGNATURES, so that a call is one zip over its arguments
_CONVERTERS = {
    name: tuple(ptr if c is vp else float if c is dbl else int if c in (i32, u32, i64) else _ref
                for c in argtypes[1:])
    for name, argtypes in {**SIGNATURES, **STREAM_SIGNATURES}.items()
    if argtypes and argtypes[0] is vp}


def _index(device):
    return device if device is None or isinstance(device, int) else device.index


def _marshal(name, converters, expected, args):
    if len(args) != expected:
        raise TypeError(f'{name} takes {expected} arguments behind the handle, got {len(args)}')
    return [c(a) for c, a in zip(converters, args)]


# handle key -> the torch stream of the last launch through that handle.  Consecutive calls carve
# their workspaces from the same slabs of the handle, so a call on another stream has to be
# ordered behind what the handle has enqueued so far (include/pbbss.h: one stream at a time).
# One entry per (device, host thread), as _handles, and as long-lived: an entry that outlives its
# handle, or is inherited with a recycled thread ident, costs the next launch one wait and no more.
_last_stream = {}


def _ordered_stream(index):
    """The current stream of the device, ordered behind the stream of the handle's previous launch
    where that was another one.  The same-stream path is one comparison and no runtime call.
    During a graph capture nothing is ordered or remembered: torch.cuda.graph has synchronised
    the device before the capture began, and the capture's private stream is gone after it.  (The
    capture query is torch's, about the current stream of the CURRENT device: a caller that
    captures on one device while launching on another is not covered.)"""
    stream = current_stream(index)
    key = (stream.device_index, threading.get_ident())
    last = _last_stream.get(key)
    # the handles of the two streams, not the objects: torch.Stream answers False to `!= None`
    if (last is None or last.cuda_stream != stream.cuda_stream) and not is_capturing():
        if last is not None:
            stream.wait_stream(last)
        _last_stream[key] = stream
    return stream


def launch(name, device, *args, what=None, accept=()):
    """Call an export whose first parameter is the handle and whose last is the stream: this
    thread's handle of `device` (a torch.device or an index), `args` marshalled slot by slot from
    SIGNATURES[name] or STREAM_SIGNATURES[name] (pointer slots: None, a contiguous device tensor or
    a ctypes object; option structs by reference; scalars through int() / float()), the current
    torch stream of the device read now and ordered behind the stream of the handle's previous
    launch.  Raises through check(rc, what or name) unless rc is in `accept`; returns rc."""
    index = _index(device)
    converters = _CONVERTERS[name]
    argv = _marshal(name, converters, len(converters) - 1, args)
    stream = _ordered_stream(index)
    rc = getattr(load(), name)(handle(index), *argv, stream_ptr(index, stream))
    if rc != OK and rc not in accept:
        check(rc, what or name)
    return rc


def launch_stream(entry, device, *args, **kw):
    """`launch` for the second table: STREAM_SIGNATURES['pbbss_<entry>_stream'] ('stft', 'istft'),
    the exports of include/pbbss_stream.h.  They take the handle and the stream like every launch
    but no memory of the handle; the ordering of `launch` behind the handle's previous stream is
    kept all the same, since their inputs usually come from calls that do."""
    name = f'pbbss_{entry}_stream'
    if name not in STREAM_SIGNATURES:
        raise KeyError(f'{name} is no export of include/pbbss_stream.h')
    return launch(name, device, *args, **kw)


def control(name, device_index, *args, what=None):
    """As launch, for the exports that take the handle but no stream (settings, read-outs, the
    communicator)."""
    converters = _CONVERTERS[name]
    argv = _marshal(name, converters, len(converters), args)
    rc = getattr(load(), name)(handle(_index(device_index)), *argv)
    if rc != OK:
        check(rc, what or name)
    return rc


# ---- host <-> device plumbing ---------------------------------------------------
def is_torch(x):
    return type(x).__module__.startswith('torch')


def to_device(x, dtype=None, device=None):
    """numpy array or torch tensor -> contiguous cuda tensor of `dtype`."""
    t = require_gpu()
    if device is None:
        device = t.device('cuda', t.cuda.current_device())
    if is_torch(x):
        out = x.to(device=device, dtype=dtype) if dtype is not None else x.to(device)
    else:
        arr = np.ascontiguousarray(x)
        out = t.from_numpy(arr).to(device)
        if dtype is not None and out.dtype != dtype:
            out = out.to(dtype)
    return out.contiguous()


def to_host(x):
    return x.detach().cpu().numpy()
