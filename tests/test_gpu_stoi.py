"""GPU: `pbbss_resample_poly` and `evaluation.stoi` against the float64 restatement of
tests/oracle_stoi.py (which tests/test_stoi_oracle.py holds against the recorded values of the
`pystoi` package).

Bounds.  Resampler: 1e-13 of the row's largest sample.  STOI: 1e-9 absolute -- d lies in
[-1, 1], and 1e-9 is what the project set for the SRMR chain of the same build (a transform,
energies, a ratio).  The frame counts before and after the removal are integers and compared
exactly.  The bound is stated for inputs whose frame energies keep 1e-6 dB from the 40 dB
threshold and whose reference segments have a centred norm above 1e-6 of their norm;
tests/test_stoi_oracle.py asserts both for every case generated here.

Observed on an MI355X: d at most 2.2e-16 from the restatement over every case here (3.3e-16 over
the 64 000-sample rows of tools/bench_stoi.py), every frame count equal; the resampler at most
3.2e-16 of the largest sample (5/4, N = 300, both input types); DESIGN 4.16.

Row lengths at 10 kHz: 4 096 samples are 30 frames and 29 STFT frames (no segment), 4 097 the
first length with a segment, 4 224 / 4 225 the next step of the frame count; `gaps` has silent
stretches at both ends and inside, with one kept frame between two removed ones (the three
source frames of an STFT frame are then three different places); `sparse` keeps 31 frames of 155;
`long` has 1 170 frames, five tiles of the selection's prefix sum, and more than 64 workgroups of
segments, so that the last sum takes a second round.
"""
import numpy as np
import pytest

import oracle_stoi as ost

pytestmark = pytest.mark.gpu

ATOL = 1e-9
RESAMPLE_TOL = 1e-13


def _torch():
    import torch
    return torch


def dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def check(got, want, what):
    got, want = host(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape)
    error = float(np.max(np.abs(got - want))) if want.size else 0.0
    print(f'{what}: largest difference {error:.3e}')
    assert error <= ATOL, (what, error)


# ---- the resampler ---------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('rate', [8000, 16000, 12000, 44100])  # 5/4, 5/8, 5/6, 100/441
def test_resample_poly(rate, dtype):
    from pb_bss_amd.evaluation import module_stoi
    up, down = ost.resample_ratio(rate)
    window = ost.resample_window(up, down)
    for N in (1, 7, 300, 3001):
        x = np.random.default_rng(N + rate).standard_normal((2, N)).astype(dtype)
        got = host(module_stoi.resample_rows(dev(x), up, down))
        want = ost.resample_poly(x.astype(np.float64), up, down, window)
        assert got.dtype == np.float64 and got.shape == want.shape == (2, -(-N * up // down))
        error = np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(x), axis=1))
        print(f'{up}/{down} N={N} {np.dtype(dtype).name}: {error:.3e} of the largest sample')
        assert error <= RESAMPLE_TOL, (rate, N, error)


# ---- 10 kHz: no resampler ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cases():
    out = {}
    for name, (x, y) in ost.cases_10k().items():
        d, frames = ost.stoi_10k(x, y, details=True)
        out[name] = (x, y, d, frames)
    return out


@pytest.mark.parametrize('name', list(ost.cases_10k()))
def test_stoi_10k(name, cases):
    from pb_bss_amd.evaluation import module_stoi, stoi
    x, y, want, want_frames = cases[name]
    out, frames = module_stoi.stoi_rows(dev(x), dev(y), 1, 1, (0, 0, 0, 0), return_frames=True)
    assert tuple(host(frames).reshape(2)) == want_frames, name
    check(out.reshape(()), want, name)
    got = stoi(x, y, ost.FS)  # NumPy in, a NumPy scalar out
    assert isinstance(got, np.float64)
    check(got, want, name + ' (public)')
    if want == ost.SHORT:
        assert got == ost.SHORT


def test_rows_of_one_call_and_twice():
    """rows with different kept counts in one call, along the outer and along the inner axis of
    the C interface; the two calls bit-identical"""
    from pb_bss_amd.evaluation import module_stoi
    N = 6000
    x, y = ost.gen_mixed_rows(11, N)
    want, want_frames = ost.stoi(x, y, ost.FS, details=True)
    xd, yd = dev(x), dev(y)
    out, frames = module_stoi.stoi_rows(xd, yd, 3, 1, (N, 0, N, 0), return_frames=True)
    assert host(frames).reshape(3, 2).tolist() == want_frames.tolist()
    check(out.reshape(3), want, 'three rows')
    again = module_stoi.stoi_rows(xd, yd, 1, 3, (0, N, 0, N))
    assert host(again).tobytes() == host(out).tobytes()


# ---- with the resampler --------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=[(8000, 5000), (16000, 8000)], ids=['8k', '16k'])
def matrix(request):
    rate, N = request.param
    reference, estimation = ost.gen_matrix(7, N)
    return rate, reference, estimation, ost.stoi(reference, estimation, rate)


def test_score_matrix_broadcast(matrix):
    from pb_bss_amd.evaluation import stoi
    rate, reference, estimation, want = matrix
    got = stoi(reference, estimation, rate)  # (2, 1, N) against (1, 3, N)
    assert isinstance(got, np.ndarray) and got.shape == (2, 3)
    check(got, want, f'(2, 3) matrix at {rate}')
    # the transposed form, and the pairs written out
    check(stoi(reference.transpose(1, 0, 2), estimation.transpose(1, 0, 2), rate), want.T,
          'transposed form')
    r, e = np.broadcast_arrays(reference, estimation)
    check(stoi(r, e, rate), want, 'written out')


def test_tensors_views_and_float32(matrix):
    from pb_bss_amd.evaluation import stoi
    t = _torch()
    rate, reference, estimation, want = matrix
    r, e = dev(reference), dev(estimation)
    t.cuda.synchronize()
    got = stoi(r, e, rate)
    assert t.is_tensor(got) and got.device == r.device and got.dtype == t.float64
    check(got, want, 'tensors')
    assert host(stoi(r, e, rate)).tobytes() == host(got).tobytes()  # bit-identical
    # a strided view (every second sample of a longer buffer) and a transposed one
    N = reference.shape[-1]
    wide = t.zeros((2, 1, 2 * N), dtype=t.float64, device=r.device)
    wide[..., ::2] = r
    turned = e[0].t().contiguous().t()  # (3, N) with strides (1, 3)
    assert wide[..., ::2].stride(-1) == 2 and turned.stride() == (1, 3)
    check(stoi(wide[..., ::2], turned[None], rate), want, 'views')
    # float32: widened, so the restatement of the rounded rows is the reference
    r32, e32 = reference.astype(np.float32), estimation.astype(np.float32)
    got32 = stoi(dev(r32), dev(e32), rate)
    assert got32.dtype == t.float64
    check(got32, ost.stoi(r32.astype(np.float64), e32.astype(np.float64), rate), 'float32')
    # one tensor on the host: the result goes where the first tensor lives
    assert stoi(t.from_numpy(reference), e, rate).device.type == 'cpu'


@pytest.mark.parametrize('rate,N', [(8000, 5000), (16000, 8000)])
def test_rows_with_different_kept_counts_and_a_zero_row(rate, N):
    from pb_bss_amd.evaluation import module_stoi, stoi
    x, y = ost.gen_mixed_rows(11, N)
    want, want_frames = ost.stoi(x, y, rate, details=True)
    assert want_frames[0, 1] != want_frames[1, 1] and want[2] == 0.0  # 0 / (0 + EPS)
    got = stoi(x, y, rate)
    check(got, want, f'mixed rows at {rate}')
    assert got[2] == want[2]
    up, down = ost.resample_ratio(rate)
    x10, y10 = (module_stoi.resample_rows(dev(v), up, down) for v in (x, y))
    M = x10.shape[-1]
    _, frames = module_stoi.stoi_rows(x10, y10, 3, 1, (M, 0, M, 0), return_frames=True)
    assert host(frames).reshape(3, 2).tolist() == want_frames.tolist()


def test_argument_checks():
    from pb_bss_amd.evaluation import stoi
    x = np.zeros(5000)
    with pytest.raises(TypeError):
        stoi(x.astype(np.complex128), x, 10000)
    with pytest.raises(ValueError):
        stoi(np.zeros((2, 0)), np.zeros((2, 0)), 10000)
    for rate in (0, -8000, 8000.5):
        with pytest.raises(ValueError):
            stoi(x, x, rate)
    assert stoi(np.zeros((0, 5000)), x, 8000).shape == (0,)
    assert stoi(x[:100], x[:100], 8000) == ost.SHORT
