"""`GriffinLim` and `MISI` of ``pb_bss/transform/griffin_lim_module.py``: iterative phase
reconstruction from the magnitudes of an STFT, on the device.

After a mask has been applied the magnitudes of a separated source are trusted and its phase is
not.  Griffin-Lim alternates between the time domain and the STFT domain, keeping the given
magnitudes and the phase the last time signal had; MISI does the same for the K sources of a
mixture `y` and distributes what their sum misses of `y` over them before every transform.

One iteration is two launches of ``csrc/griffin_lim.hip`` (analysis window, forward FFT,
magnitude projection, inverse FFT and synthesis window of a frame without leaving LDS, then a
deterministic overlap-add that also forms the MISI correction); ``step(iterations=n)`` enqueues
all ``2 n`` of them in one C call.  NumPy in gives NumPy attributes, a device tensor gives device
tensors, enqueued on the current stream without a host synchronisation.

Beyond the reference: ``step(iterations=n)``, and leading independent axes -- `X` (..., K, T, F)
with `y` (..., n) -- served in one launch chain.  A complex64 `X` is widened exactly; its
magnitudes are formed in float64 (``numpy.abs`` of a complex64 array would round them to
float32).
"""
from functools import partial

import numpy as np

from .. import _lib, engine
from .stft import analysis_window, biorthogonal_window, istft, stft, stft_frames_to_samples

__all__ = ['GriffinLim', 'MISI']

_FIRST_GUESSES = ('istft', 'white_gaussian_noise', 'y')
_WINDOW = 'blackman'  # the default of stft / istft: the reference class passes no window


def _home(X):
    """the device a tensor `X` lives on; None (the current one) for host data"""
    return X.device if _lib.is_torch(X) and X.is_cuda else None


class GriffinLim:
    """
    @article{Griffin1984GriffinLim,
      title={Signal estimation from modified short-time Fourier transform},
      author={Griffin, Daniel and Lim, Jae},
      journal={IEEE Transactions on Acoustics, Speech, and Signal Processing},
      volume={32},
      number={2},
      pages={236--243},
      year={1984},
      publisher={IEEE}
    }

    `X` (K, T, F) holds the magnitudes (its phase is ignored after the first guess), F =
    size // 2 + 1.  Attributes as in the reference: `X`, `y`, `x_hat` (K, n) -- the current time
    signals, n = T * shift + size - shift without fading --, `X_dash_dash` (the STFT of what the
    last step transformed) and `X_dash` (the same with the magnitudes of `X`); the two are `X`
    itself before the first step.

    `first_guess`: ``'istft'`` (``istft(X)``), ``'y'`` (``y / K`` for every source) or
    ``'white_gaussian_noise'`` (``numpy.random.randn`` on the host; the reference's own line
    passes ``size=`` to ``randn`` and raises ``TypeError``, this one draws the noise).  Anything
    else raises ``ValueError(first_guess)``.  Where `y` is used -- by ``first_guess='y'`` and
    by `MISI` -- it has to be there (``TypeError``) and to have the n samples of `x_hat`
    (``ValueError``; the reference fails to broadcast in its first step).
    """
    _needs_y = False

    def __init__(
            self,
            X: 'Shape: (K, T, F)',
            y: 'Shape: (num_samples,)' = None,
            first_guess='istft',
            size=512, shift=128, fading=False,
    ):
        if first_guess not in _FIRST_GUESSES:
            raise ValueError(first_guess)
        shape = tuple(X.shape)
        if len(shape) < 3:
            raise ValueError(f'X has to be (..., K, T, F), got shape {shape}')
        lead, (K, T, F) = shape[:-3], shape[-3:]
        if size < 4 or size & (size - 1) or shift < 1 or size % shift:
            raise ValueError(f'size={size} has to be a power of two and a multiple of shift={shift}')
        if F != size // 2 + 1 or K < 1 or T < 1:
            raise ValueError(f'X {shape} is not (..., K, T, size // 2 + 1 = {size // 2 + 1})')
        samples = stft_frames_to_samples(T, size, shift, fading=fading)
        if self._needs_y or first_guess == 'y':
            if y is None:
                raise TypeError(f'{type(self).__name__}(first_guess={first_guess!r}) needs y')
            if tuple(y.shape) != lead + (samples,):
                raise ValueError(
                    f'y {tuple(y.shape)} does not match the {T} frames of X: x_hat is '
                    f'{lead + (K, samples)}, y has to be {lead + (samples,)}')

        self.size, self.shift, self.fading = size, shift, fading
        self.stft = partial(stft, size=size, shift=shift, fading=fading)
        self.istft = partial(istft, size=size, shift=shift, fading=fading)

        self.X = X
        self.X_dash_dash = X
        self.X_dash = X
        self.y = y
        self._like_torch = _lib.is_torch(X)
        self._resident = {}  # attribute -> (the object it held, its device tensor)
        self._windows = None  # (analysis, synthesis) on the device

        if first_guess == 'istft':
            self.x_hat = self.istft(X)
        elif first_guess == 'white_gaussian_noise':
            noise = np.random.randn(*lead, K, samples)
            self.x_hat = _lib.to_device(noise, device=_home(X)) if self._like_torch else noise
        else:
            # Text just under [Gunawan2010MISI] Equation 5
            if self._like_torch:
                # a tensor divisor: by a Python number torch multiplies with the reciprocal,
                # which is not y / K in the last bit
                t = _lib.torch()
                yd = _lib.to_device(y, t.float64, device=_home(X))
                divisor = t.full((K, 1), K, dtype=t.float64, device=yd.device)
                self.x_hat = yd.unsqueeze(-2) / divisor
            else:
                yh = _lib.to_host(y) if _lib.is_torch(y) else np.asarray(y, dtype=np.float64)
                self.x_hat = np.repeat(yh[..., None, :] / K, K, axis=-2)

    def _device(self, name, dtype=None):
        """the attribute `name` as a contiguous device tensor; a host array is sent once"""
        value = getattr(self, name)
        held = self._resident.get(name)
        if held is not None and held[0] is value:
            return held[1]
        t = _lib.torch()
        tensor = _lib.to_device(value, device=_home(self.X))
        if dtype is None:
            if tensor.dtype not in (t.complex64, t.complex128):
                tensor = tensor.to(t.complex128)
        elif tensor.dtype != dtype:
            tensor = tensor.to(dtype)
        self._resident[name] = (value, tensor)
        return tensor

    def _iterate(self, iterations, y):
        iterations = int(iterations)
        if iterations < 1:
            raise ValueError(f'iterations={iterations}: at least one')
        t = _lib.torch()
        X = self._device('X')
        x_hat = self._device('x_hat', t.float64)
        lead, (K, T, F) = tuple(X.shape[:-3]), tuple(X.shape[-3:])
        if tuple(x_hat.shape) != lead + (K, x_hat.shape[-1]):
            raise ValueError(f'x_hat {tuple(x_hat.shape)} does not belong to X {tuple(X.shape)}')
        B = int(np.prod(lead, dtype=np.int64))
        if y is not None and tuple(y.shape) != lead + (x_hat.shape[-1],):
            raise ValueError(f'y {tuple(y.shape)} does not belong to x_hat {tuple(x_hat.shape)}')
        if self._windows is None or self._windows[0].device != X.device:
            window = analysis_window(_WINDOW, self.size)
            self._windows = tuple(_lib.to_device(w, t.float64, device=X.device)
                                  for w in (window, biorthogonal_window(window, self.shift)))
        aw, sw = self._windows
        out, X_dash_dash, X_dash = engine.griffin_lim(
            X.reshape(B, K, T, F), None if y is None else y.reshape(B, -1),
            x_hat.reshape(B, K, -1), self.size, self.shift, aw, sw, fading=self.fading,
            iterations=iterations)
        out = out.reshape(lead + (K, -1))
        X_dash_dash = X_dash_dash.reshape(lead + (K, T, F))
        X_dash = X_dash.reshape(lead + (K, T, F))
        if self._like_torch:
            self.x_hat, self.X_dash_dash, self.X_dash = out, X_dash_dash, X_dash
        else:
            self.x_hat = _lib.to_host(out)
            self.X_dash_dash, self.X_dash = _lib.to_host(X_dash_dash), _lib.to_host(X_dash)
        self._resident['x_hat'] = (self.x_hat, out)

    def step(self, iterations=1):
        """One iteration, as the reference's `step`; `iterations=n`: n of them in one call, with
        `X_dash_dash` and `X_dash` those of the last one."""
        self._iterate(iterations, None)

    def evaluate(self, speech_source):
        """

        Args:
            speech_source: Oracle for evaluation, (K, n).

        Returns: dict with the mean BSS-Eval SDR and SIR of `x_hat` and the inconsistency of
            `X_dash`: the power of what `stft(istft(.))` changes in it.

        """
        from ..evaluation import OutputMetrics
        from ..evaluation.sxr_module import get_variance_for_zero_mean_signal

        metrics = OutputMetrics(
            speech_prediction=self.x_hat,
            speech_source=speech_source,
            enable_si_sdr=True,
        )

        return dict(
            mir_eval_sdr=metrics.mir_eval['sdr'].mean(),
            mir_eval_sir=metrics.mir_eval['sir'].mean(),
            inconsistency=get_variance_for_zero_mean_signal(
                self.X_dash - self.stft(self.istft(self.X_dash))
            )
        )


class MISI(GriffinLim):
    """
    @article{Gunawan2010MISI,
      title={Iterative phase estimation for the synthesis of separated sources from single-channel mixtures},
      author={Gunawan, David and Sen, Deep},
      journal={IEEE Signal Processing Letters},
      volume={17},
      number={5},
      pages={421--424},
      year={2010},
      publisher={IEEE}
    }

    `y` (n,) is the mixture the K sources of `X` add up to, at most 8 of them.
    """
    _needs_y = True

    def step(self, iterations=1):
        """One iteration: the error ``e = y - sum_k x_hat[k]`` (equation 5) is spread evenly,
        ``x_hat + e / K`` (equation 4), before the transform, the projection (equation 3) and
        the inverse transform (equation 2).  `iterations=n` as in `GriffinLim.step`."""
        self._iterate(iterations, self._device('y', _lib.torch().float64))
