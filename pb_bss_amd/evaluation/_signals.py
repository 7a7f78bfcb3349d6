"""Host plumbing shared by the evaluation metrics: time signals to the device and back."""
import numpy as np

from .. import _lib

SPAN = 4096  # samples of a row one workgroup owns (csrc/eval.hpp: kEvalSpan)


def device_signal(x, complex_ok):
    """NumPy array, sequence or torch tensor -> device tensor of float32 / float64 (complex64 /
    complex128 where `complex_ok`), strides untouched for a device tensor.  Integers and
    booleans become float64, as NumPy's true division makes them."""
    t = _lib.require_gpu()
    if _lib.is_torch(x):
        if not x.is_cuda:
            x = x.to(t.device('cuda', t.cuda.current_device()))
    else:
        arr = np.asarray(x)
        if arr.dtype.kind in 'biu':
            arr = arr.astype(np.float64)
        x = t.from_numpy(np.ascontiguousarray(arr)).to(t.device('cuda', t.cuda.current_device()))
    if x.dtype in (t.float32, t.float64):
        return x
    if x.dtype in (t.complex64, t.complex128):
        if not complex_ok:
            raise TypeError(f'complex signal ({x.dtype}) where a real one is expected')
        return x
    if not x.dtype.is_floating_point and not x.dtype.is_complex:
        return x.to(t.float64)
    raise TypeError(f'signal must be float32/64 or complex64/128, not {x.dtype}')


def common_dtype(a, b):
    """both tensors in the type the pair promotes to (a copy only where they differ)"""
    t = _lib.torch()
    dtype = t.promote_types(a.dtype, b.dtype)
    return a.to(dtype), b.to(dtype)


def dtype_code(x):
    t = _lib.torch()
    return {t.float32: _lib.EVAL_F32, t.float64: _lib.EVAL_F64, t.complex64: _lib.EVAL_C64,
            t.complex128: _lib.EVAL_C128}[x.dtype]


def home_of(*signals):
    """(like_torch, device a tensor result goes to): the first tensor argument decides"""
    for s in signals:
        if _lib.is_torch(s):
            return True, s.device
    return False, None


def result(out, like_torch, home):
    """tensor on `home`, or NumPy (a 0-d result as a NumPy scalar, as the reference returns)"""
    if like_torch:
        return out if out.device == home else out.to(home)
    return _lib.to_host(out)[()]


def collapse(axes):
    """axes: [(size, stride_a, stride_b)] slowest first -> the merged axes (size-1 axes dropped,
    neighbours merged where both strides allow)"""
    merged = []
    for size, sa, sb in axes:
        if size == 1:
            continue
        if merged:
            psize, psa, psb = merged[-1]
            if psa == sa * size and psb == sb * size:
                merged[-1] = (psize * size, sa, sb)
                continue
        merged.append((size, sa, sb))
    return merged
