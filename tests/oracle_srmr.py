"""Float64 restatement of the reference's SRMR (pb_bss/evaluation/module_srmr.py) and gammatone
filterbank (pb_bss/transform/gammatone.py): serial filters (scipy.signal.lfilter), the envelope
through an FFT of the row's own length, frames cut and windowed as the reference does.

Also the zero-padding `segment_axis` stub that stands in for the reference's one outside import
(and the tail-cutting one it is told apart from), `load_reference`, which imports the unmodified
reference files, and the seeded cases the CPU and GPU tests share.
"""
import cmath
import importlib.util
import math
import os
import sys
import types

import numpy as np
from scipy.signal import lfilter

MODULATION_FREQUENCIES = [4.0, 6.5, 10.7, 17.6, 28.9, 47.5, 78.1, 128.0]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'srmr.npz')


# ---- framing ----------------------------------------------------------------------------------
def segment_axis_pad(x, length, shift, axis=-1, end='pad'):
    """frames of `length` samples, `shift` apart; the last, partial frame is filled with zeros"""
    x = np.asarray(x)
    assert x.ndim == 1 and axis in (-1, 0)
    frames = max(-(-(len(x) - length) // shift), 0) + 1
    padded = np.zeros((frames - 1) * shift + length, dtype=x.dtype)
    padded[:len(x)] = x
    return np.stack([padded[f * shift:f * shift + length] for f in range(frames)])


def segment_axis_cut(x, length, shift, axis=-1, end='cut'):
    """the same without the partial frame at the end"""
    x = np.asarray(x)
    assert x.ndim == 1 and axis in (-1, 0)
    frames = (len(x) - length) // shift + 1 if len(x) >= length else 0
    return np.stack([x[f * shift:f * shift + length] for f in range(frames)])


def load_reference(segment_axis=segment_axis_pad):
    """(module_srmr, gammatone) of the unmodified reference, framing with `segment_axis`"""
    from oracle import refshim
    refshim.load()
    root = os.path.join(refshim.REFERENCE_ROOT, 'pb_bss')
    if 'pb_bss.transform' not in sys.modules:  # the package's own __init__ imports Griffin-Lim
        package = types.ModuleType('pb_bss.transform')
        package.__path__ = [os.path.join(root, 'transform')]
        sys.modules['pb_bss.transform'] = package
    gammatone = importlib.import_module('pb_bss.transform.gammatone')
    stubs = {}
    for name in ('paderbox', 'paderbox.array', 'paderbox.array.segment'):
        stubs[name] = types.ModuleType(name)
    stubs['paderbox.array.segment'].segment_axis = segment_axis
    saved = {name: sys.modules.get(name) for name in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location(
            '_reference_module_srmr', os.path.join(root, 'evaluation', 'module_srmr.py'))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    finally:
        for name, previous in saved.items():
            if previous is None:
                del sys.modules[name]
            else:
                sys.modules[name] = previous
    return module, gammatone


# ---- the filterbank ---------------------------------------------------------------------------
def hz_to_erbs(f):
    return 21.4 * math.log(0.00437 * f + 1, 10)


def erbs_to_hz(e):
    return (10 ** (e / 21.4) - 1) / 0.00437


def centre_frequencies(low, high, n):
    lo, hi = hz_to_erbs(low), hz_to_erbs(high)
    return np.array([erbs_to_hz(lo + i * ((hi - lo) / n)) for i in range(n)])


def channel_stages(cf, sample_rate):
    """[(b, a)] of the four stages of the channel at `cf` Hz (Apple TR #35)"""
    T = 1 / sample_rate
    B = 1.019 * 2 * math.pi * (cf / 9.26449 + 24.7)
    arg = 2 * cf * math.pi * T
    damp = math.exp(B * T)
    a = [1.0, -2 * math.cos(arg) / damp, math.exp(-2 * B * T)]
    big, small = math.sqrt(3 + 2 ** 1.5), math.sqrt(3 - 2 ** 1.5)
    signed = [big, -big, small, -small]
    k1 = -2 * cmath.exp(2j * arg) * T
    k2 = 2 * cmath.exp(-B * T + 1j * arg) * T
    gain = 1.0
    for r in signed:
        gain *= abs(k1 + k2 * (math.cos(arg) + r * math.sin(arg)))
    gain /= abs(-2 / math.exp(2 * B * T) - 2 * cmath.exp(2j * arg)
                + 2 * (1 + cmath.exp(2j * arg)) / damp) ** 4
    stages = []
    for i, r in enumerate(signed):
        b = np.array([T, -(T * math.cos(arg) / damp + r * T * math.sin(arg) / damp), 0.0])
        stages.append((b / gain if i == 0 else b, a))
    return stages


def gammatone_filterbank(signal, sample_rate=16000, n=23, low_freq=125, high_freq=0):
    """(n, *signal.shape) float64"""
    signal = np.asarray(signal, dtype=np.float64)
    if high_freq == 0:
        high_freq = sample_rate / 2
    out = []
    for cf in centre_frequencies(low_freq, high_freq, n):
        y = signal
        for b, a in channel_stages(cf, sample_rate):
            y = lfilter(b, a, y, axis=-1)
        out.append(y)
    return np.stack(out)


# ---- SRMR ---------------------------------------------------------------------------------------
def vad(x, sample_rate):
    """the samples the voice activity detection keeps"""
    x = np.asarray(x)
    flagged = np.flatnonzero(np.abs(x) > np.abs(x).max() ** 2 / 1e5)
    keep = np.ones(len(x), dtype=bool)
    for first, second in zip(flagged[:-1], flagged[1:]):
        if second - first > 0.05 * sample_rate:
            keep[first + 1:second] = False
    return x[keep]


def analytic_modulus(y):
    N = len(y)
    h = np.zeros(N)
    if N % 2 == 0:
        h[0] = h[N // 2] = 1
        h[1:N // 2] = 2
    else:
        h[0] = 1
        h[1:(N + 1) // 2] = 2
    return np.abs(np.fft.ifft(np.fft.fft(y) * h))


def modulation_filters(sample_rate):
    filters = []
    for f in MODULATION_FREQUENCIES:
        w0 = math.tan(2 * math.pi * f / (2 * sample_rate))
        b0 = w0 / 2
        norm = 1 + b0 + w0 ** 2
        filters.append((np.array([b0, 0, -b0]) / norm,
                        np.array([norm, 2 * w0 ** 2 - 2, 1 - b0 + w0 ** 2]) / norm))
    return filters


def band_means(x, sample_rate=16000, n=23, low_freq=125, segment_axis=segment_axis_pad):
    """(the (n, 8) mean frame energies of one row, the number of samples the VAD kept)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        x = vad(np.asarray(x, dtype=np.float64), sample_rate)
        x = x - np.mean(x)
        x = x / np.std(x)
    bands = gammatone_filterbank(x, sample_rate, n, low_freq)
    unit = int(sample_rate / 1000)
    window = 0.54 + 0.46 * np.cos(np.linspace(-np.pi, np.pi, unit * 256))
    means = np.empty((n, 8))
    for j in range(n):
        envelope = analytic_modulus(bands[j])
        for k, (b, a) in enumerate(modulation_filters(sample_rate)):
            frames = segment_axis(lfilter(b, a, envelope), unit * 256, unit * 64)
            means[j, k] = np.mean(np.sum(np.square(window * frames), axis=-1))
    return means, len(x)


def score(means, sample_rate=16000, low_freq=125, details=None):
    """the scalar tail; details: 'cumulative' (n), 'bandwidth', 'cutoffs' (8), 'stopped_at'"""
    n = means.shape[0]
    erbs = centre_frequencies(low_freq, sample_rate / 2, n) / 9.26449 + 24.7
    cumulative = np.cumsum(means.sum(axis=1) * 100 / means.sum())
    above = np.flatnonzero(cumulative > 90)
    bandwidth = erbs[above[0]] if len(above) else 0.0
    cutoffs = [f - math.tan(2 * math.pi * f / sample_rate / 2) / 2 * sample_rate / (2 * math.pi)
               for f in MODULATION_FREQUENCIES]
    columns = means.sum(axis=0)
    denominator, stopped_at = columns[4], None
    for i in range(5, 8):
        denominator = denominator + columns[i]
        if cutoffs[i - 1] < bandwidth < cutoffs[i]:
            stopped_at = i
            break
    if details is not None:
        details.update(cumulative=cumulative, bandwidth=bandwidth, cutoffs=np.array(cutoffs),
                       stopped_at=stopped_at)
    with np.errstate(divide='ignore', invalid='ignore'):
        return columns[:4].sum() / denominator


def srmr(signal, sample_rate=16000, n=23, low_freq=125, segment_axis=segment_axis_pad,
         details=None):
    """SRMR of every row; details (a list) receives one dict per row: score()'s and 'kept'"""
    signal = np.asarray(signal)
    out = np.empty(signal.shape[:-1])
    for index in np.ndindex(*signal.shape[:-1]):
        means, kept = band_means(signal[index], sample_rate, n, low_freq, segment_axis)
        row = {'kept': kept}
        out[index] = score(means, sample_rate, low_freq, row)
        if details is not None:
            details.append(row)
    return out[()]


# ---- seeded cases -------------------------------------------------------------------------------
def doctest_signal():
    """the reference's recorded example (wrapper.py: OutputMetrics doctest): 203.3988 at 8 kHz"""
    return np.array([1., 2., 3., 4.] * 1000)


DOCTEST_VALUE, DOCTEST_RATE = 203.3988, 8000


def speechlike(seed, N, sample_rate=16000, dtype=np.float64):
    """noise under a slow envelope: spread over the cochlear channels and the modulation bands"""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / sample_rate
    envelope = 0.6 + 0.4 * np.sin(2 * np.pi * (3 + seed % 5) * t + rng.uniform(0, 6))
    return (envelope * rng.standard_normal(N)).astype(dtype)


def low_tone(seed, N, sample_rate=16000, frequency=200.0, modulation=6.0):
    """an amplitude-modulated low tone with a little noise: the energy sits in the first
    cochlear channels, the 90 % bandwidth is small and falls between two cutoffs"""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / sample_rate
    tone = (1 + 0.8 * np.sin(2 * np.pi * modulation * t)) * np.sin(2 * np.pi * frequency * t)
    return tone + 1e-3 * rng.standard_normal(N)


def with_gaps(x, gaps):
    """zeros in x[start:start + length] for every (start, length); the neighbours are made loud
    enough to be flagged.  The flagged neighbours are then length + 1 apart."""
    x = np.array(x)
    for start, length in gaps:
        x[start:start + length] = 0
        for edge in (start - 1, start + length):
            if abs(x[edge]) < 0.5:
                x[edge] = 0.5 if x[edge] >= 0 else -0.5
    return x


def batch_with_gaps(sample_rate=16000, N=5000):
    """three rows that keep different numbers of samples: 5000 (no gap), 4200 and 4096 (one
    dropped gap each).  The first use of an FFT length costs the device library a second or
    two, so the kept lengths are ones that other cases have as well."""
    width = int(0.05 * sample_rate)
    rows = [speechlike(20 + r, N, sample_rate) for r in range(3)]
    rows[1] = with_gaps(rows[1], [(1500, width)])
    rows[2] = with_gaps(rows[2], [(700, N - 4096)])
    return np.stack(rows)


def cases():
    """name -> dict(signal, sample_rate, n, low_freq): the SRMR cases of the CPU and the GPU
    tests.  The chunked filters of csrc/srmr.hip take 64 samples per lane and 4096 per
    lane-group: row lengths below 64, at 4096 and 4097, over three lane-groups, and the primes
    4099 and 8191 for the FFT."""
    width = 800  # 0.05 * 16000
    out = {}

    def add(name, signal, sample_rate=16000, n=23, low_freq=125):
        out[name] = dict(signal=signal, sample_rate=sample_rate, n=n, low_freq=low_freq)

    add('doctest', doctest_signal(), DOCTEST_RATE)
    add('below_chunk', speechlike(1, 50))
    add('one_group', speechlike(2, 4096))
    add('one_group_plus_one', speechlike(3, 4097))
    add('three_groups', speechlike(4, 9001))
    add('prime_4099_one_channel', speechlike(5, 4099), n=1)
    add('prime_4099_64_channels', speechlike(6, 4099), n=64)
    add('prime_8191_8k', speechlike(7, 8191, 8000), 8000)
    add('low_freq_200', speechlike(8, 5000), low_freq=200)
    add('float32', speechlike(9, 4097, dtype=np.float32))
    add('low_tone', low_tone(10, 9000))
    add('batch_gaps', batch_with_gaps())
    add('shape_2_3', np.stack([speechlike(30 + r, 2000) for r in range(6)]).reshape(2, 3, 2000))
    # voice activity detection
    base = speechlike(11, 5000)
    add('vad_gap_at_width', with_gaps(base, [(2000, width - 1)]))     # neighbours 800 apart: kept
    add('vad_gap_above_width', with_gaps(base, [(2000, width)]))      # 801 apart: dropped
    add('vad_two_gaps', with_gaps(base, [(800, width + 600), (3000, 2 * width)]))  # keeps 2000
    edges = np.array(base)
    edges[:1200] = 0
    edges[-1500:] = 0
    add('vad_silent_edges', edges)                                     # kept: no neighbour outside
    return out
