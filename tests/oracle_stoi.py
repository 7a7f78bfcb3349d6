"""Float64 NumPy restatement of short-time objective intelligibility (Taal et al. 2011) as the
`pystoi` package computes it behind the reference's pb_bss/evaluation/module_stoi.py, which is
not installed here.  The fixed point: the eight values the reference's own
tests/test_evaluation/test_wrapper_values.py records of the real package at sample_rate=8000
(RECORDED_INPUT at rtol=1e-5, RECORDED_OUTPUT at rtol=1e-6); tests/test_stoi_oracle.py holds this
file against them.  NumPy only: the resampler is the direct sum, so that the GPU tests need
nothing else.  Also the seeded generators shared by the CPU and the GPU tests.
"""
import importlib.util
import math
import os

import numpy as np

FS = 10000
FRAME = 256
HOP = 128
NFFT = 512
BANDS = 15
MIN_FREQ = 150.0
SEGMENT = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = np.finfo(float).eps
SHORT = 1e-5  # the value of a row with fewer than SEGMENT STFT frames

# tests/test_evaluation/test_wrapper_values.py of the reference, sample_rate=8000
RECORDED_INPUT = [[0.691546, 0.626544, 0.717809], [0.28424, 0.345368, 0.279996]]
RECORDED_OUTPUT = [0.968833, 0.976151]
RECORDED_INPUT_RTOL = 1e-5
RECORDED_OUTPUT_RTOL = 1e-6

WINDOW = np.hanning(FRAME + 2)[1:-1]


def load_reference_scenario():
    """`scenario` of the reference's tests/test_evaluation/test_wrapper_values.py, by path;
    the module's top imports pb_bss.evaluation.wrapper, which is given a stand-in"""
    import sys
    import types
    from oracle import refshim
    path = os.path.join(refshim.REFERENCE_ROOT, 'tests', 'test_evaluation',
                        'test_wrapper_values.py')
    names = ('pb_bss', 'pb_bss.evaluation', 'pb_bss.evaluation.wrapper')
    saved = {name: sys.modules.get(name) for name in names}
    for name in names:
        sys.modules[name] = types.ModuleType(name)
    sys.modules['pb_bss.evaluation.wrapper'].InputMetrics = None
    sys.modules['pb_bss.evaluation.wrapper'].OutputMetrics = None
    try:
        spec = importlib.util.spec_from_file_location('_reference_test_wrapper_values', path)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    finally:
        for name, previous in saved.items():
            if previous is None:
                del sys.modules[name]
            else:
                sys.modules[name] = previous
    return module.scenario


def load_reference_stoi():
    """module_stoi.stoi of the unmodified reference, by path (it imports pystoi only when called)"""
    from oracle import refshim
    path = os.path.join(refshim.REFERENCE_ROOT, 'pb_bss', 'evaluation', 'module_stoi.py')
    spec = importlib.util.spec_from_file_location('_reference_module_stoi', path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.stoi


# ---- 1. the resampler -------------------------------------------------------------------------
def resample_ratio(sample_rate):
    g = math.gcd(FS, int(sample_rate))
    return FS // g, int(sample_rate) // g


def resample_window(up, down):
    """(2 L + 1) taps of Octave's `resample`: a Kaiser-windowed sinc, unit sum"""
    fc = 1.0 / (2 * max(up, down))
    rejection = 60.0
    half = int(math.ceil((rejection - 8.0) / (28.714 * fc / 10)))
    t = np.arange(-half, half + 1)
    ideal = 2 * up * fc * np.sinc(2 * fc * t)
    h = np.kaiser(2 * half + 1, 0.1102 * (rejection - 8.7)) * ideal
    return h / np.sum(h)


def resample_poly(x, up, down, window):
    """out[m] = up * sum_n x[n] window[L + m down - n up], m < ceil(len up / down): the direct sum"""
    x = np.asarray(x, np.float64)
    n_in = x.shape[-1]
    half = (len(window) - 1) // 2
    n_out = -(-n_in * up // down)
    m = np.arange(n_out, dtype=np.int64)
    first = -((half - m * down) // up)  # ceil((m down - L) / up)
    taps = 2 * half // up + 1
    n = first[:, None] + np.arange(taps, dtype=np.int64)
    k = half + m[:, None] * down - n * up
    valid = (k >= 0) & (k <= 2 * half) & (n >= 0) & (n < n_in)
    w = np.where(valid, window[np.clip(k, 0, 2 * half)], 0.0)
    xv = x[..., np.clip(n, 0, max(n_in - 1, 0))]
    return up * np.sum(xv * w, axis=-1)


# ---- 2. silent frames -------------------------------------------------------------------------
def frame_starts(length):
    return np.arange(0, length - FRAME, HOP)


def frame_energies(x):
    """20 log10(||w x_f|| + EPS) of every frame of the reference row"""
    starts = frame_starts(len(x))
    frames = x[starts[:, None] + np.arange(FRAME)] * WINDOW
    return 20 * np.log10(np.linalg.norm(frames, axis=1) + EPS)


def remove_silent_frames(x, y):
    """-> (x, y without the frames 40 dB below the loudest of x, frames before, frames after)"""
    starts = frame_starts(len(x))
    if len(starts) == 0:
        return np.zeros(0), np.zeros(0), 0, 0
    energies = frame_energies(x)
    keep = (np.max(energies) - DYN_RANGE - energies) < 0
    kept = starts[keep]
    xo = np.zeros((len(kept) - 1) * HOP + FRAME)
    yo = np.zeros_like(xo)
    for k, s in enumerate(kept):
        xo[k * HOP:k * HOP + FRAME] += x[s:s + FRAME] * WINDOW
        yo[k * HOP:k * HOP + FRAME] += y[s:s + FRAME] * WINDOW
    return xo, yo, len(starts), len(kept)


# ---- 3. / 4. the transform and the bands ------------------------------------------------------
def band_edges():
    """(15, 2) first and one-past-last bin of every third-octave band"""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    i = np.arange(BANDS)
    low = MIN_FREQ * 2.0 ** ((2 * i - 1) / 6)
    high = MIN_FREQ * 2.0 ** ((2 * i + 1) / 6)
    return np.stack([np.argmin(np.abs(f[None] - low[:, None]), axis=1),
                     np.argmin(np.abs(f[None] - high[:, None]), axis=1)], axis=1)


def band_matrix():
    obm = np.zeros((BANDS, NFFT // 2 + 1))
    for i, (lo, hi) in enumerate(band_edges()):
        obm[i, lo:hi] = 1
    return obm


def third_octave_bands(x):
    """(T, 15): sqrt of the band sums of |rfft|^2 over the Hann frames of x"""
    starts = frame_starts(len(x))
    frames = x[starts[:, None] + np.arange(FRAME)] * WINDOW
    power = np.abs(np.fft.rfft(frames, n=NFFT, axis=1)) ** 2
    return np.sqrt(power @ band_matrix().T)


# ---- 5. the segments ---------------------------------------------------------------------------
def segments(tob):
    """(T, 15) -> (J, 15, 30), J = T - 29"""
    T = tob.shape[0]
    index = np.arange(T - SEGMENT + 1)[:, None] + np.arange(SEGMENT)
    return tob[index].transpose(0, 2, 1)


def centred_norm_ratio(x_tob):
    """the smallest centred norm of a reference segment band over its plain norm (the condition the
    GPU bound is stated for); inf where there is no segment"""
    if x_tob.shape[0] < SEGMENT:
        return np.inf
    xs = segments(x_tob)
    centred = np.linalg.norm(xs - xs.mean(axis=-1, keepdims=True), axis=-1)
    plain = np.linalg.norm(xs, axis=-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(plain > 0, centred / plain, np.inf)
    return float(np.min(ratio))


def correlate(x_tob, y_tob):
    xs, ys = segments(x_tob), segments(y_tob)
    c = np.linalg.norm(xs, axis=-1, keepdims=True) / (np.linalg.norm(ys, axis=-1, keepdims=True) + EPS)
    yp = np.minimum(ys * c, xs * (1 + 10 ** (-BETA / 20)))
    yp = yp - yp.mean(axis=-1, keepdims=True)
    xs = xs - xs.mean(axis=-1, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=-1, keepdims=True) + EPS)
    xs = xs / (np.linalg.norm(xs, axis=-1, keepdims=True) + EPS)
    return float(np.sum(yp * xs) / (xs.shape[0] * BANDS))


# ---- the metric ---------------------------------------------------------------------------------
def stoi_10k(x, y, details=False):
    """one pair of rows at 10 kHz -> d (details: also the frames before and after the removal)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    xs, ys, before, after = remove_silent_frames(x, y)
    d = SHORT
    if after - 1 >= SEGMENT:
        d = correlate(third_octave_bands(xs), third_octave_bands(ys))
    return (d, (before, after)) if details else d


def stoi(reference, estimation, sample_rate, details=False):
    """broadcasting pairs of rows -> d of every pair (details: also int (..., 2) frame counts)"""
    reference, estimation = np.broadcast_arrays(np.asarray(reference, np.float64),
                                                np.asarray(estimation, np.float64))
    lead = reference.shape[:-1]
    out = np.empty(lead)
    frames = np.empty(lead + (2,), np.int64)
    up, down = resample_ratio(sample_rate)
    window = resample_window(up, down) if sample_rate != FS else None
    cache = {}

    def at_10k(row):
        if window is None:
            return row
        key = row.tobytes()
        if key not in cache:
            cache[key] = resample_poly(row, up, down, window)
        return cache[key]

    for index in np.ndindex(*lead):
        out[index], frames[index] = stoi_10k(at_10k(reference[index]), at_10k(estimation[index]),
                                             details=True)
    return (out[()], frames) if details else out[()]


# ---- seeded cases --------------------------------------------------------------------------------
def gen_pair(seed, N, snr_db=5.0):
    """amplitude-modulated noise and a noisy copy of it"""
    rng = np.random.default_rng(seed)
    t = np.arange(N)
    clean = rng.standard_normal(N) * (1.0 + 0.8 * np.sin(2 * np.pi * t / 1500.0 + seed))
    noisy = clean + 10 ** (-snr_db / 20) * rng.standard_normal(N)
    return clean, noisy


def gen_gaps(seed, N=12000, island_frame=35):
    """noise under a gain of 1 or 1e-4: silent stretches at both ends and inside, and inside the
    interior one 20 loud samples at the centre of frame `island_frame`, where the window of both
    neighbours is below -40 dB: one kept frame between two removed ones"""
    clean, noisy = gen_pair(seed, N)
    gain = np.ones(N)
    gain[:600] = 1e-4           # leading
    gain[-700:] = 1e-4          # trailing
    gain[3900:5300] = 1e-4      # interior ...
    centre = island_frame * HOP + FRAME // 2
    gain[centre - 10:centre + 10] = 1.0  # ... with the island
    return clean * gain, noisy * gain


def gen_sparse(seed, N=20000, loud=(6000, 6000 + 30 * HOP)):
    """a row of many frames of which only those that touch `loud` are kept"""
    clean, noisy = gen_pair(seed, N)
    gain = np.full(N, 1e-5)
    gain[loud[0]:loud[1]] = 1.0
    return clean * gain, noisy * gain


def cases_10k():
    """name -> (x, y) at 10 kHz: the frame counts around the first segment, a row too short for a
    frame, silent stretches, a row that keeps 31 frames of 155, and a row of 15 s: 1 170 frames
    (the selection's prefix sum runs over five tiles of 256, the first of them with removed
    frames) and more than 64 workgroups of segments (the last sum takes two rounds)"""
    cases = {f'n{N}': gen_pair(N, N) for N in (4096, 4097, 4224, 4225)}
    cases['short'] = gen_pair(5, 200)
    cases['gaps'] = gen_gaps(3)
    cases['sparse'] = gen_sparse(4)
    cases['long'] = gen_gaps(6, 150000)
    return cases


def gen_matrix(seed, N, sources=2, sensors=3):
    """reference (sources, 1, N) and estimation (1, sensors, N): mixtures of the sources"""
    rng = np.random.default_rng(seed)
    clean = np.stack([gen_pair(seed + k, N)[0] for k in range(sources)])
    mix = rng.uniform(0.2, 1.0, (sensors, sources)) @ clean + 0.1 * rng.standard_normal((sensors, N))
    return clean[:, None, :], mix[None, :, :]


def gen_mixed_rows(seed, N):
    """(3, N) pairs that keep different numbers of frames; the last pair is all zeros"""
    a = gen_pair(seed, N)
    b = gen_pair(seed + 1, N)
    gain = np.ones(N)
    gain[N // 3:N // 2] = 1e-4
    zero = np.zeros(N)
    return np.stack([a[0], b[0] * gain, zero]), np.stack([a[1], b[1] * gain, zero])


def conditions(x, y, sample_rate=FS):
    """(distance in dB of the nearest frame energy from the 40 dB threshold, smallest centred over
    plain norm of a reference segment band) of one pair: what the bound of the device test is
    stated for"""
    if sample_rate != FS:
        up, down = resample_ratio(sample_rate)
        window = resample_window(up, down)
        x, y = resample_poly(x, up, down, window), resample_poly(y, up, down, window)
    xs, _, _, _ = remove_silent_frames(np.asarray(x, np.float64), np.asarray(y, np.float64))
    return threshold_margin(x), centred_norm_ratio(third_octave_bands(xs))


def threshold_margin(x):
    """smallest distance in dB of a frame energy of x from the 40 dB threshold"""
    if len(frame_starts(len(x))) == 0:
        return np.inf
    e = frame_energies(x)
    return float(np.min(np.abs(np.max(e) - DYN_RANGE - e)))
