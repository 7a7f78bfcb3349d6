"""Float64 restatement of the reference's oracle masks (pb_bss/extraction/mask_module.py) that
also reports how well determined each binary decision is.

The threshold masks compare row values with an order statistic; a device result can only be
demanded to equal the reference entry for entry where no value sits within rounding distance of
a decision.  `lorenz_mask` and `quantile_mask` here take a `details` dict and fill in the
margins; `assert_lorenz_determined` / `assert_quantile_determined` are the preconditions the GPU
tests state before they compare.
"""
import numpy as np

EPS = 1e-18
MARGIN = 1e-9

NAMES = [
    'voiced_unvoiced_split_characteristic', 'ideal_binary_mask', 'wiener_like_mask',
    'ideal_ratio_mask', 'ideal_amplitude_mask', 'phase_sensitive_mask', 'ideal_complex_mask',
    'lorenz_mask', 'quantile_mask', 'biased_binary_mask',
]


def gen(seed, shape):
    """Heavy-tailed complex64 images: (N + iN) N^2 elementwise."""
    rng = np.random.default_rng(seed)
    a, b, c = (rng.standard_normal(shape) for _ in range(3))
    return ((a + 1j * b) * c ** 2).astype(np.complex64)


def gen_integer(seed, shape):
    """Integer-valued images: every power and sum is exact, ties are real ties."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, shape) + 1j * rng.integers(-3, 4, shape)).astype(np.complex64)


def _power(x, sensor_axis):
    p = x.real ** 2 + x.imag ** 2
    if sensor_axis is not None:
        p = p.sum(sensor_axis, keepdims=True)
    return p


def _squeeze(m, sensor_axis, keepdims):
    if sensor_axis is not None and not keepdims:
        m = np.squeeze(m, sensor_axis)
    return m


def ideal_binary_mask(x, source_axis=0, sensor_axis=None, keepdims=False):
    x = np.asarray(x)
    p = _power(x, sensor_axis)
    best = np.expand_dims(np.argmax(p, axis=source_axis), source_axis)
    shape = [1] * x.ndim
    shape[source_axis] = x.shape[source_axis]
    m = best == np.arange(x.shape[source_axis]).reshape(shape)
    return _squeeze(m, sensor_axis, keepdims).astype(x.real.dtype)


def ibm_ties(x, source_axis=0, sensor_axis=None):
    """number of points at which two sources share the largest pooled power"""
    p = _power(np.asarray(x), sensor_axis)
    return int(((p == p.max(source_axis, keepdims=True)).sum(source_axis) > 1).sum())


def wiener_like_mask(x, source_axis=0, sensor_axis=None, eps=EPS, keepdims=False):
    p = _power(np.asarray(x), sensor_axis)
    return _squeeze(p / (p.sum(source_axis, keepdims=True) + eps), sensor_axis, keepdims)


def ideal_ratio_mask(x, source_axis=0, eps=EPS):
    m = np.abs(np.asarray(x))
    return m / (m.sum(source_axis, keepdims=True) + eps)


def ideal_amplitude_mask(x, source_axis=0, eps=EPS):
    x = np.asarray(x)
    return np.abs(x) / (np.abs(x.sum(source_axis, keepdims=True)) + eps)


def phase_sensitive_mask(x, source_axis=0, eps=EPS):
    x = np.asarray(x)
    o = x.sum(source_axis, keepdims=True)
    return np.abs(x) / (np.abs(o) + eps) * np.cos(np.angle(x) - np.angle(o))


def ideal_complex_mask(x, source_axis=0):
    x = np.asarray(x)
    with np.errstate(invalid='ignore', divide='ignore'):
        return x / x.sum(source_axis, keepdims=True)


def amplification(x, source_axis=0, eps=EPS):
    """max(1, |s| / (|sum s| + eps)): the factor by which the unbounded masks (amplitude,
    phase-sensitive, complex) scale the rounding error of the observed sum"""
    x = np.asarray(x)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.maximum(1.0, np.abs(x) / (np.abs(x.sum(source_axis, keepdims=True)) + eps))


def _rows(v, axis):
    """(rows, N) view of v with `axis` flattened last, and the inverse"""
    axis = tuple(a % v.ndim for a in (axis if isinstance(axis, (tuple, list)) else (axis,)))
    keep = [a for a in range(v.ndim) if a not in axis]
    perm = keep + list(axis)
    moved = np.transpose(v, perm)
    shape = moved.shape
    rows = int(np.prod(shape[:len(keep)], dtype=np.int64))

    def back(m):
        return np.transpose(m.reshape(shape), np.argsort(perm))

    return moved.reshape(rows, -1), back


def lorenz_mask(x, *, sensor_axis=None, axis=(-2, -1), lorenz_fraction=0.98, weight=0.999,
                keepdims=False, details=None):
    x = np.asarray(x)
    p = np.abs(x) ** 2
    if sensor_axis is not None:
        p = p.sum(axis=sensor_axis, keepdims=True)
    rows, back = _rows(p, axis)
    m = np.zeros_like(rows)
    margins, down = [], 0
    for i, row in enumerate(rows):
        srt = np.sort(row)[::-1]
        lorenz = np.cumsum(srt) / np.sum(srt)
        below = lorenz < lorenz_fraction
        if not below.any():
            raise ValueError(f'row {i}: no element below the Lorenz fraction')
        m[i] = row > srt[below].min()
        margins.append(float(np.abs(lorenz - lorenz_fraction).min()))
        down += int((m[i] == 0).sum())
    if details is not None:
        details['margin'] = min(margins)
        details['down'] = down
        details['up'] = int(rows.size - down)
    m = back(0.5 + weight * (m - 0.5))
    return _squeeze(m, sensor_axis, keepdims)


def assert_lorenz_determined(details):
    assert details['margin'] >= MARGIN, details


def quantile_mask(x, quantile=(0.1, -0.9), *, axis=-2, weight=0.999, details=None):
    v = np.abs(np.asarray(x))
    if isinstance(quantile, (tuple, list)):
        parts = []
        for q in quantile:
            d = {}
            parts.append(quantile_mask(v, q, axis=axis, weight=weight, details=d))
            if details is not None:
                details['gap'] = min(details.get('gap', np.inf), d['gap'])
                details['equal'] = details.get('equal', 0) + d['equal']
        return np.array(parts)
    rows, back = _rows(v, axis)
    q = (1 - quantile) * 100 if quantile >= 0 else abs(quantile) * 100
    thr = np.percentile(rows, q=q, axis=-1)[:, None]
    m = (rows > thr if quantile >= 0 else rows < thr).astype(rows.dtype)
    if details is not None:
        rel = np.abs(rows - thr) / np.maximum(np.abs(thr), np.finfo(np.float64).tiny)
        equal = rows == thr
        details['equal'] = int(equal.sum())
        details['gap'] = float(rel[~equal].min()) if (~equal).any() else np.inf
    return back(0.5 + weight * (m - 0.5))


def assert_quantile_determined(details):
    """every value is bit-equal to its row's threshold or at least MARGIN (relative) away"""
    assert details['gap'] >= MARGIN, details


def voiced_unvoiced_split_characteristic(frequency_bins, split_bin=None, width=None):
    if split_bin is None:
        split_bin = frequency_bins // 2
    if width is None:
        width = frequency_bins // 5
    k = np.arange(width)
    voiced = np.ones(frequency_bins)
    start = int(split_bin - width / 2)
    voiced[start - 1:start + width - 1] = 0.5 * (1 + np.cos(np.pi / (width - 1) * k))
    voiced[start - 1 + width:] = 0
    return voiced, 1 - voiced


def biased_binary_mask(x, component_axis=0, threshold_unvoiced_speech=5,
                       threshold_voiced_speech=0, threshold_unvoiced_noise=-10,
                       threshold_voiced_noise=-10, low_cut=5, high_cut=500, details=None):
    """thresholds and cuts along the last axis; the upper cut ends at the length of axis 1 of
    the masks, as the reference has it"""
    x = np.asarray(x)
    assert x.shape[component_axis] == 2
    voiced, unvoiced = voiced_unvoiced_split_characteristic(x.shape[-1])
    ts = threshold_voiced_speech * voiced + threshold_unvoiced_speech * unvoiced
    tn = threshold_unvoiced_noise * voiced + threshold_voiced_noise * unvoiced
    p = x.real ** 2 + x.imag ** 2
    speech, noise = np.split(p, 2, axis=component_axis)
    ps, pn = speech / 10 ** (ts / 10), speech / 10 ** (tn / 10)
    ms = (ps > noise) & (ps > 0.005)
    mn = (pn < noise) | (pn < 0.005)
    end = ms.shape[1]
    ms[..., 0:low_cut - 1] = 0
    ms[..., high_cut:end] = 0
    mn[..., 0:low_cut - 1] = 1
    mn[..., high_cut:end] = 1
    if details is not None:
        # smallest relative distance of a compared pair: the decisions are safe against one
        # rounding of the quotient when it is far above 1e-15
        tiny = np.finfo(np.float64).tiny
        gaps = [np.abs(a - b) / np.maximum(np.abs(b), tiny)
                for a, b in ((ps, noise), (pn, noise), (ps, 0.005 + 0 * ps), (pn, 0.005 + 0 * pn))]
        details['gap'] = float(min(g.min() for g in gaps))
    return np.concatenate([ms, mn], axis=component_axis)
