"""Streaming `stft` / `istft`: the two ends of the frame-recursive chain (``OnlineWPE`` ->
``OnlineCACGMM`` -> ``OnlineMVDR``), audio block in -> frames, frames -> audio block out, with the
state on the device and one kernel launch per call (``pb_bss_amd/csrc/stft_stream.hip``).

The contract is that of the other online stages: any blocking gives bit for bit what one call
gives.  For a signal ``x`` cut into blocks of any lengths, the concatenation of every
``OnlineSTFT.step_block`` result and of ``flush(pad)`` IS ``stft(x, ..., pad=pad)``, and the
concatenation of every ``OnlineISTFT.step_block`` result and of ``flush()`` IS ``istft(X, ...)`` of
the concatenated frames -- the same bits, not merely close values: a frame goes through the
windowing, FFT and untangling statements of the offline kernel, and an output sample adds its
covering frames from 0.0 in ascending frame order, as the offline overlap-add does.

State.  ``OnlineSTFT`` keeps the last ``window_length - 1`` samples per channel as float64 on the
device (the ``window_length - shift`` samples every next frame overlaps plus fewer than ``shift``
pending ones; widening float32 is exact, so float32 and float64 blocks may alternate) in two
buffers whose roles flip with every call, and ``samples_seen`` / ``frames_seen`` as host integers,
from which the number of frames a call returns follows without reading anything back.
``OnlineISTFT`` keeps the overlap tail ``(rows, window_length - shift)`` float64 on the device and
``frames_seen`` on the host.

Algorithmic latency of the pair: ``window_length - shift`` samples (a sample leaves the inverse
when the last frame covering it has arrived) plus the block.
"""
import numpy as np

from .. import _lib, engine
from .stft import analysis_window, biorthogonal_window

__all__ = ['OnlineSTFT', 'OnlineISTFT', 'OnlineSTFTState', 'OnlineISTFTState']


def _served(size, window_length, shift):
    """The range of the offline transforms (csrc/stft.hip): what lies outside raises as they do."""
    if size < 4 or size & (size - 1) or size > 8192 or not 1 <= window_length <= size:
        raise NotImplementedError(
            f'size = {size}, window_length = {window_length}: served for size a power of two in '
            '[4, 8192] and window_length <= size')
    assert shift >= 1, shift


class OnlineSTFTState:
    """``history`` (channels, max(1, window_length - 1)) float64 on the device: the samples
    behind the stream, newest last, zeros in front of its start; ``samples_seen`` and
    ``frames_seen``: host integers."""

    def __init__(self, history, samples_seen=0, frames_seen=0):
        self.history, self.samples_seen, self.frames_seen = history, samples_seen, frames_seen

    def clone(self):
        return OnlineSTFTState(self.history.clone(), self.samples_seen, self.frames_seen)


class OnlineSTFT:
    """``stft`` of a stream of sample blocks (module docstring).  The arguments are those of
    `stft`; ``layout='f t d'`` (the default: what the mixture models and the online stages read)
    returns (F, m, channels), ``layout=None`` (channels, m, F)."""

    def __init__(self, channels, size=1024, shift=256, window='blackman', window_length=None,
                 fading=True, symmetric_window=False, *, layout='f t d', dtype=None, state=None):
        t = _lib.require_gpu()
        wl = size if window_length is None else window_length
        _served(size, wl, shift)
        if layout is not None and layout.replace(' ', '') != 'ftd':
            raise ValueError(f"layout must be None or 'f t d', got {layout!r}")
        if fading and wl < shift:
            raise ValueError(f'fading needs window_length {wl} >= shift {shift}')
        assert channels >= 1, channels
        self.channels, self.size, self.shift, self.window_length = channels, size, shift, wl
        self.fading, self.layout, self.dtype = bool(fading), layout, dtype
        self._args = dict(window=window, symmetric_window=symmetric_window)
        self._c128 = dtype is None or np.dtype(dtype) == np.complex128
        device = (t.device('cuda', t.cuda.current_device()) if state is None
                  else state.history.device)
        self._window = _lib.to_device(analysis_window(window, wl, symmetric_window), t.float64,
                                      device=device)
        H = max(1, wl - 1)
        if state is None:
            state = OnlineSTFTState(t.zeros((channels, H), dtype=t.float64, device=device))
        else:
            assert tuple(state.history.shape) == (channels, H) and \
                state.history.dtype == t.float64, (tuple(state.history.shape), state.history.dtype)
            state = state.clone()
        # [0]: the samples behind the stream, [1]: what the next call writes; flipped per call
        self._history = [state.history.contiguous(), t.empty_like(state.history)]
        self.samples_seen, self.frames_seen = int(state.samples_seen), int(state.frames_seen)
        self._like_torch = True

    # ---- state ---------------------------------------------------------------------------------
    history = property(lambda self: self._history[0])

    def state(self):
        """A copy of the stream's state (`from_state` continues from it)."""
        return OnlineSTFTState(self._history[0].clone(), self.samples_seen, self.frames_seen)

    @classmethod
    def from_state(cls, state, size=1024, shift=256, window='blackman', window_length=None,
                   fading=True, symmetric_window=False, *, layout='f t d', dtype=None):
        """A stream that continues behind ``state`` (which is not modified); the transform's
        arguments must be those of the stream the state comes from."""
        return cls(state.history.shape[0], size, shift, window, window_length, fading,
                   symmetric_window, layout=layout, dtype=dtype, state=state)

    def clone(self):
        """Fork the stream: an independent object in the same state."""
        return type(self).from_state(self.state(), self.size, self.shift,
                                     window_length=self.window_length, fading=self.fading,
                                     layout=self.layout, dtype=self.dtype, **self._args)

    # ---- the stream ----------------------------------------------------------------------------
    def _launch(self, x, n, m, flush):
        out = engine.stft_stream(x, n, self._history[0], self._history[1], self.samples_seen,
                                 self.frames_seen, m, self.size, self.shift, self._window,
                                 fading=self.fading, flush=flush,
                                 layout=0 if self.layout is None else 1, out_c128=self._c128)
        self._history.reverse()
        return out if self._like_torch else _lib.to_host(out)

    def step_block(self, samples):
        """samples (channels, n) -> the frames these samples complete, (F, m, channels) or
        (channels, m, F); m may be 0.  One kernel launch, no host read-back for tensor input."""
        t = _lib.torch()
        self._like_torch = _lib.is_torch(samples)
        x = _lib.to_device(samples, device=self._window.device)
        if x.dtype not in (t.float32, t.float64):
            x = x.to(t.float64)
        assert x.ndim == 2 and x.shape[0] == self.channels, (tuple(x.shape), self.channels)
        n = int(x.shape[1])
        fade = self.window_length - self.shift if self.fading else 0
        total = fade + self.samples_seen + n
        complete = 0 if total < self.window_length else (total - self.window_length) // self.shift + 1
        m = complete - self.frames_seen
        if n == 0:  # nothing moves: no launch, no flip
            F = self.size // 2 + 1
            out = t.empty((self.channels, 0, F) if self.layout is None else (F, 0, self.channels),
                          dtype=t.complex128 if self._c128 else t.complex64, device=x.device)
            return out if self._like_torch else _lib.to_host(out)
        out = self._launch(x, n, m, False)
        self.samples_seen += n
        self.frames_seen += m
        return out

    def flush(self, pad=True):
        """The remaining frames of the stream that ends here -- the closing fade and, with
        ``pad``, the zero-padded last frame --; afterwards the object is in its initial state."""
        T = _lib.load().pbbss_stft_num_frames(self.samples_seen, self.size, self.shift,
                                              self.window_length, int(self.fading), int(bool(pad)))
        if T < 0:
            _lib.check(T, 'stft_num_frames')
        m = max(0, T - self.frames_seen)
        out = self._launch(None, 0, m, True)
        self.samples_seen = self.frames_seen = 0
        return out


class OnlineISTFTState:
    """``tail`` (rows, window_length - shift) float64 on the device: the sums behind the last
    complete hop; ``frames_seen``: host integer; ``lead``: the leading axes of the stream."""

    def __init__(self, tail, frames_seen=0, lead=None):
        self.tail, self.frames_seen = tail, frames_seen
        self.lead = (tail.shape[0],) if lead is None else tuple(lead)

    def clone(self):
        return OnlineISTFTState(self.tail.clone(), self.frames_seen, self.lead)


class OnlineISTFT:
    """``istft`` of a stream of frame blocks (module docstring).  The arguments are those of
    `istft`.  ``step_block(frames (..., m, F))``, or ``(..., F, m)`` with ``layout='f t'`` (read
    through its strides: what ``OnlineMVDR.step_block`` returns, stacked over the classes), gives
    ``(..., s)`` float64: one hop of ``shift`` samples per frame, less the first
    ``window_length - shift`` samples of the stream with ``fading`` (as `istft` drops them).  The
    leading axes are independent rows, fixed by the first call."""

    def __init__(self, size=1024, shift=256, window='blackman', window_length=None, fading=True,
                 symmetric_window=False, *, layout=None, state=None):
        _lib.require_gpu()
        wl = size if window_length is None else window_length
        if layout is not None and layout.replace(' ', '') != 'ft':
            raise ValueError(f"layout must be None or 'f t', got {layout!r}")
        # raises ValueError for window_length % shift != 0
        self._synthesis = biorthogonal_window(analysis_window(window, wl, symmetric_window), shift)
        _served(size, wl, shift)
        self.size, self.shift, self.window_length = size, shift, wl
        self.fading, self.layout = bool(fading), layout
        self._args = dict(window=window, symmetric_window=symmetric_window)
        self._window = None          # the synthesis window on the stream's device
        self._tail = self._lead = None
        self.frames_seen = 0
        self._like_torch = True
        if state is not None:
            t = _lib.torch()
            state = state.clone()
            rows = int(np.prod(state.lead, dtype=np.int64))
            assert tuple(state.tail.shape) == (rows, wl - shift) and \
                state.tail.dtype == t.float64, (tuple(state.tail.shape), state.lead)
            self._open(state.lead, state.tail.device)
            self._tail, self.frames_seen = state.tail.contiguous(), int(state.frames_seen)

    # ---- state ---------------------------------------------------------------------------------
    tail = property(lambda self: self._tail)

    def _open(self, lead, device):
        t = _lib.torch()
        self._lead = tuple(lead)
        rows = int(np.prod(self._lead, dtype=np.int64))
        self._window = _lib.to_device(self._synthesis, t.float64, device=device)
        self._tail = t.zeros((rows, self.window_length - self.shift), dtype=t.float64,
                             device=device)

    def state(self):
        """A copy of the stream's state; None before the first call (no rows yet)."""
        if self._tail is None:
            return None
        return OnlineISTFTState(self._tail.clone(), self.frames_seen, self._lead)

    @classmethod
    def from_state(cls, state, size=1024, shift=256, window='blackman', window_length=None,
                   fading=True, symmetric_window=False, *, layout=None):
        """A stream that continues behind ``state`` (which is not modified)."""
        return cls(size, shift, window, window_length, fading, symmetric_window, layout=layout,
                   state=state)

    def clone(self):
        """Fork the stream: an independent object in the same state."""
        return type(self).from_state(self.state(), self.size, self.shift,
                                     window_length=self.window_length, fading=self.fading,
                                     layout=self.layout, **self._args)

    # ---- the stream ----------------------------------------------------------------------------
    def step_block(self, frames):
        """frames (..., m, F) -- (..., F, m) with ``layout='f t'`` -- -> (..., s) float64 samples.
        One kernel launch, no scratch, no host read-back."""
        t = _lib.torch()
        self._like_torch = _lib.is_torch(frames)
        X = frames if self._like_torch and frames.is_cuda else _lib.to_device(frames)
        if X.dtype not in (t.complex64, t.complex128):
            X = X.to(t.complex128)
        assert X.ndim >= 2, tuple(X.shape)
        if self.layout is not None:
            X = X.transpose(-1, -2)
        F = self.size // 2 + 1
        assert X.shape[-1] == F, f'frequency axis {X.shape[-1]} != size // 2 + 1 = {F}'
        lead, m = tuple(X.shape[:-2]), int(X.shape[-2])
        if self._tail is None:
            self._open(lead, X.device)
        assert lead == self._lead, (lead, self._lead)
        X = X.to(self._tail.device)
        rows = self._tail.shape[0]
        fade = self.window_length - self.shift if self.fading else 0
        skip = max(0, fade - self.frames_seen * self.shift)
        if m == 0 or rows == 0:
            out = t.empty((rows, 0), dtype=t.float64, device=self._tail.device)
        else:
            out = engine.istft_stream(X.reshape(rows, m, F), self.size, self.shift, self._window,
                                      self._tail, skip)
            self.frames_seen += m
        out = out.reshape(lead + (out.shape[-1],))
        return out if self._like_torch else _lib.to_host(out)

    def flush(self):
        """The tail of the stream that ends here: (..., window_length - shift) without fading,
        empty with it (`istft` drops it); afterwards the object is in its initial state."""
        t = _lib.torch()
        lead = self._lead if self._lead is not None else ()
        if self._tail is None:
            n = 0 if self.fading else self.window_length - self.shift
            out = t.zeros(lead + (n,), dtype=t.float64, device='cuda')
        elif self.fading:
            out = self._tail.new_empty(lead + (0,))
        else:
            out = self._tail.reshape(lead + (self._tail.shape[-1],))  # handed over, not copied
        self._tail = self._lead = None
        self.frames_seen = 0
        return out if self._like_torch else _lib.to_host(out)
