"""`InputMetrics` and `OutputMetrics` (interface of the reference's pb_bss/evaluation/wrapper.py):
every metric of one utterance behind one object, each computed on first use and kept.

The metrics this package computes on the device are there: BSS-Eval (`mir_eval_sdr`, `_sir`,
`_sar`, `_selection`), `si_sdr` and the invasive SxR.  `pesq` and `stoi` wrap third-party
packages that are not available; they raise NotImplementedError and are listed as disabled
instead of available.  So does `srmr` here, for now: the package computes it
(`pb_bss_amd.evaluation.srmr`, which needs no clean source), the two classes are not wired to it
yet.  Arrays go in as NumPy arrays or device tensors and the metrics come back in kind.

Both classes are thin: `_Metrics` holds the table of metric names, the dict views and the
properties that only pick a key out of a grouped result; a subclass says which signals it got,
checks their shapes and supplies the three grouped results (`mir_eval`, `invasive_sxr`,
`si_sdr`).
"""
import difflib
import functools

import numpy as np

from .. import _lib
from . import _signals
from .module_mir_eval import mir_eval_sources
from .module_si_sdr import si_sdr
from .sxr_module import input_sxr, output_sxr

__all__ = ['InputMetrics', 'OutputMetrics', 'VerboseKeyError']

# metric -> the package the reference computes it with
_UNWRAPPED = {'pesq': 'pesq', 'stoi': 'pystoi', 'srmr': 'srmrpy'}
_INVASIVE = ('invasive_sdr', 'invasive_snr', 'invasive_sir')
_MAX_SPEAKERS = 8           # of sources and of targets (the selection search)
_MAX_INVASIVE_SOURCES = 4   # the reference admits fewer than 5 sources with contributions
_MAX_DEVIATION = 1e-3       # of the prediction from the sum of its contributions
_NOT_THERE = object()


class VerboseKeyError(KeyError):
    """KeyError(item, keys[, note]): the message names the keys closest to `item` first"""

    def __str__(self):
        if not 2 <= len(self.args) <= 3:
            return super().__str__()
        item, keys, *note = self.args
        ranked = difflib.get_close_matches(item, keys, cutoff=0, n=100)
        return '\n'.join([f'{item!r}.', f'Close matches: {ranked!r}', *map(str, note)])


def _require(holds, message):
    """the shape checks raise AssertionError, as the reference's asserts do, also under -O"""
    if not holds:
        raise AssertionError(message)


def _picked(name, key):
    """cached property that takes `key` out of the grouped result `name`"""
    def pick(self):
        return getattr(self, name)[key]
    pick.__name__ = f'{name}_{key}'
    return functools.cached_property(pick)


def _unwrapped(name):
    def refuse(self):
        raise NotImplementedError(
            f'{name} is computed by the package {_UNWRAPPED[name]!r} in the reference; '
            f'pb_bss_amd does not wrap that package')
    refuse.__name__ = name
    return functools.cached_property(refuse)


def _take(array, selection):
    """array[selection] along the first axis, for arrays and tensors in any combination"""
    if _lib.is_torch(array):
        index = _lib.torch().as_tensor(selection, device=array.device)
        return array.index_select(0, index)
    if _lib.is_torch(selection):
        selection = _lib.to_host(selection)
    return np.asarray(array)[np.asarray(selection)]


class _Metrics:
    enable_si_sdr = False
    _with_invasive = False                 # were the signals of the invasive SxR given?
    _always = ('mir_eval_sdr', 'mir_eval_sir', 'mir_eval_sar')

    pesq, stoi, srmr = (_unwrapped(name) for name in _UNWRAPPED)
    mir_eval_sdr = _picked('mir_eval', 'sdr')
    mir_eval_sir = _picked('mir_eval', 'sir')
    mir_eval_sar = _picked('mir_eval', 'sar')
    invasive_sdr = _picked('invasive_sxr', 'sdr')
    invasive_sir = _picked('invasive_sxr', 'sir')
    invasive_snr = _picked('invasive_sxr', 'snr')

    def _optional(self):
        """[(metric names, are they switched on)]"""
        return [(('si_sdr',), self.enable_si_sdr), (_INVASIVE, self._with_invasive)]

    def _available_metric_names(self):
        return self._always + tuple(
            name for names, on in self._optional() if on for name in names)

    def _disabled_metric_names(self):
        return list(_UNWRAPPED) + [
            name for names, on in self._optional() if not on for name in names]

    def as_dict(self):
        return {name: self[name] for name in self._available_metric_names()}

    def __getitem__(self, item):
        if not isinstance(item, str):
            raise AssertionError(f'a metric is named by a str, not by {type(item).__name__}: '
                                 f'{item!r}')
        value = getattr(self, item, _NOT_THERE)
        if value is _NOT_THERE:
            raise VerboseKeyError(item, self._available_metric_names(),
                                  f'Disabled: {self._disabled_metric_names()}')
        return value

    def _need_si_sdr_enabled(self):
        if not self.enable_si_sdr:
            raise ValueError(
                'si_sdr is switched off unless asked for: it means something for a single '
                'channel without reverberation only. Pass `enable_si_sdr=True` to get it.')


class InputMetrics(_Metrics):
    def __init__(
            self,
            observation: 'Shape(D, N)',
            speech_source: 'Shape(K_source, N)',
            speech_image: 'Shape(K_source, D, N)'=None,
            noise_image: 'Shape(D, N)'=None,
            sample_rate: int = None,
            enable_si_sdr: bool = False,
    ):
        """The metrics of the unprocessed `observation` (D, N): each of the D channels against
        each of the K_source rows of `speech_source`, so every metric has the shape
        (K_source, D).  Pass a single channel (1, N) to score a reference channel only.

        `speech_image` (K_source, D, N) and `noise_image` (D, N), both or neither, enable the
        invasive SxR.  `enable_si_sdr`: SI-SDR is meaningful for non-reverberant single-channel
        data only and therefore off by default.  `sample_rate` is kept for the metrics that need
        it; none of those is available here.
        """
        self.enable_si_sdr = enable_si_sdr
        self.sample_rate = sample_rate
        self.observation, self.speech_source = observation, speech_source
        self.speech_image, self.noise_image = speech_image, noise_image
        self._has_image_signals = self._with_invasive = not (
            speech_image is None or noise_image is None)
        self.K_source = speech_source.shape[0]
        self.channels, self.samples = observation.shape[-2:]
        self.check_inputs()

    def check_inputs(self):
        for name in ('observation', 'speech_source'):
            shape = tuple(getattr(self, name).shape)
            _require(len(shape) == 2, f'{name} has to be a matrix (rows, N), got shape {shape}')

    @functools.cached_property
    def mir_eval(self):
        # Every channel is scored against the same sources.  They are handed over once, with a
        # stride of zero along the channels, so they are correlated and factorised once.
        like_torch, home = _signals.home_of(self.speech_source, self.observation)
        source = _signals.device_signal(self.speech_source, complex_ok=False)
        observation = _signals.device_signal(self.observation, complex_ok=False).to(source.device)
        full = (self.K_source, self.channels, self.samples)
        scores = mir_eval_sources(
            reference=source[:, None, :].expand(full),
            estimation=observation[None, :, :].expand(full),
            return_dict=True,
            compute_permutation=False,
        )
        return {name: _signals.result(value, like_torch, home) for name, value in scores.items()}

    @functools.cached_property
    def invasive_sxr(self):
        return input_sxr(self.speech_image, self.noise_image, average_sources=False,
                         average_channels=False, return_dict=True)

    @functools.cached_property
    def si_sdr(self):
        # (sources, 1, N) against (1, channels, N): the (K_source, D) score matrix
        self._need_si_sdr_enabled()
        return si_sdr(reference=self.speech_source[:, None, :],
                      estimation=self.observation[None, :, :])


class OutputMetrics(_Metrics):
    _always = _Metrics._always + ('mir_eval_selection',)

    def __init__(
            self,
            speech_prediction: 'Shape(K_target, N)',
            speech_source: 'Shape(K_source, N)',
            speech_contribution: 'Shape(K_source, K_target, N)'=None,
            noise_contribution: 'Shape(K_target, N)'=None,
            sample_rate: int = None,
            enable_si_sdr: bool = False,
            compute_permutation: bool = True,
    ):
        """The metrics of a separation system's output.

        `speech_prediction` (K_target, N) holds the estimates, `speech_source` (K_source, N) the
        true sources before reverberation; K_target is K_source or K_source + 1 (a noise
        estimate), both at most 8.  With `compute_permutation` the estimates are assigned to the
        sources by the largest mean BSS-Eval SIR (`mir_eval_selection`) and every other metric
        uses that assignment; without it estimate k belongs to source k.

        `speech_contribution` (K_source, K_target, N) and `noise_contribution` (K_target, N),
        both or neither, enable the invasive SxR.  They exist for linear systems only: apply
        the enhancement of every target to every source image and to the noise alone; their sum
        has to reproduce `speech_prediction`.  `enable_si_sdr`: see `InputMetrics`.

        >>> metrics = OutputMetrics(
        ...     speech_prediction=np.array([[1., 2., 3., 4.] * 1000, [4., 3., 2., 1.] * 1000]),
        ...     speech_source=np.array([[1., 2., 2., 3., 2.] * 800, [4., 3., 3., 2., 3.] * 800]))
        >>> metrics.mir_eval_sdr.round(4), metrics.mir_eval_selection  # doctest: +SKIP
        (array([7.2565, 7.3303]), array([0, 1]))
        """
        self.enable_si_sdr = enable_si_sdr
        self.compute_permutation = compute_permutation
        self.sample_rate = sample_rate
        self.speech_prediction, self.speech_source = speech_prediction, speech_source
        self.speech_contribution = speech_contribution
        self.noise_contribution = noise_contribution
        self._has_contribution_signals = self._with_invasive = not (
            speech_contribution is None or noise_contribution is None)
        self.K_target, self.samples = speech_prediction.shape[0], speech_prediction.shape[-1]
        self.K_source = speech_source.shape[0]
        self.check_inputs()

    def _shapes(self):
        """the shapes that were given next to the ones that are expected"""
        expected = {
            'speech_prediction': '(K_target, N)', 'speech_source': '(K_source, N)',
            'speech_contribution': '(K_source, K_target, N)',
            'noise_contribution': '(K_target, N)'}
        lines = [f'  {name}: {tuple(getattr(self, name).shape)}, expected {symbols}'
                 for name, symbols in expected.items() if getattr(self, name) is not None]
        return '\n'.join(['Shapes given:'] + lines)

    def check_inputs(self):
        def require(holds, message):
            _require(holds, f'{message}\n{self._shapes()}')

        for name in ('speech_prediction', 'speech_source'):
            shape = tuple(getattr(self, name).shape)
            _require(len(shape) == 2, f'{name} has to be a matrix (rows, N), got shape {shape}')
        for count, name in ((self.K_source, 'speech_source'), (self.K_target, 'speech_prediction')):
            require(count <= _MAX_SPEAKERS,
                    f'{name} has {count} rows; at most {_MAX_SPEAKERS} speakers are scored.')
        require(0 <= self.K_target - self.K_source <= 1,
                f'{self.K_target} predictions for {self.K_source} sources: there has to be one '
                f'per source, or one more (the noise).')
        require(self.speech_source.shape[1] == self.samples,
                'speech_source and speech_prediction differ in their number of samples.')

        given = [s is not None for s in (self.speech_contribution, self.noise_contribution)]
        _require(all(given) or not any(given),
                 'speech_contribution and noise_contribution belong together: give both or '
                 f'neither (got speech_contribution={self.speech_contribution!r}, '
                 f'noise_contribution={self.noise_contribution!r}).')
        if not all(given):
            return
        require(tuple(self.speech_contribution.shape[1:]) == (self.K_target, self.samples),
                'speech_contribution needs one row of N samples per target in each source.')
        require(self.K_source <= _MAX_INVASIVE_SOURCES,
                f'the invasive SxR takes at most {_MAX_INVASIVE_SOURCES} sources, as in the '
                f'reference; speech_source has {self.K_source}.')
        require(tuple(self.noise_contribution.shape) == (self.K_target, self.samples),
                'noise_contribution needs one row of N samples per target.')
        rest = self.speech_prediction - self.speech_contribution.sum(0) - self.noise_contribution
        if _lib.is_torch(rest):
            deviation = float(rest.abs().double().std(unbiased=False))
        else:
            deviation = float(np.std(np.abs(rest)))
        _require(deviation < _MAX_DEVIATION,
                 f'speech_prediction is not the sum of its contributions: the magnitude of the '
                 f'rest has a standard deviation of {deviation} (limit {_MAX_DEVIATION}).')

    @functools.cached_property
    def mir_eval(self):
        return mir_eval_sources(
            reference=self.speech_source,
            estimation=self.speech_prediction,
            return_dict=True,
            compute_permutation=self.compute_permutation,
        )

    @functools.cached_property
    def mir_eval_selection(self):
        if self.compute_permutation:
            return self.mir_eval['selection']
        _require(self.K_target == self.K_source,
                 f'without the search, prediction k is scored against source k: '
                 f'{self.K_target} predictions do not pair up with {self.K_source} sources.')
        if _lib.is_torch(self.speech_source):
            return _lib.torch().arange(self.K_source, device=self.speech_source.device)
        return np.arange(self.K_source)

    @functools.cached_property
    def speech_prediction_selection(self):
        """the K_source predictions the selection assigns to the sources, in source order"""
        return _take(self.speech_prediction, self.mir_eval_selection)

    @functools.cached_property
    def invasive_sxr(self):
        selection = self.mir_eval_selection
        contribution = self.speech_contribution
        if _lib.is_torch(contribution):
            per_target = _take(contribution.transpose(0, 1), selection).transpose(0, 1)
        else:
            per_target = np.moveaxis(_take(np.moveaxis(contribution, 1, 0), selection), 0, 1)
        return output_sxr(per_target, _take(self.noise_contribution, selection),
                          average_sources=False, return_dict=True)

    @functools.cached_property
    def si_sdr(self):
        self._need_si_sdr_enabled()
        return si_sdr(reference=self.speech_source, estimation=self.speech_prediction_selection)
