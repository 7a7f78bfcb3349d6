"""GPU: `evaluation.srmr` and `transform.gammatone_filterbank` against the recorded outputs of
the reference (tests/golden/srmr.npz) and the float64 restatement (tests/oracle_srmr.py).

Tolerances.  SRMR values: relative 1e-9.  The restatement with chunked filters and per-sample
frame weights is within 1.5e-11 of the reference on the host; the device adds the tree-shaped
carry over the lanes and fused multiply-adds, for which a factor of about 60 is allowed.
Filterbank output: 1e-9 of the channel's peak.  The kept lengths of the voice activity
detection are integers and compared exactly.

Observed on an MI355X: SRMR at most 1.4e-11 relative (`shape_2_3`), filterbank at most 1.4e-13
of the peak (64 channels); DESIGN 4.14.  With the powers of the state matrix in plain float64
the 64-channel case measured 1.2e-9: they are computed in double-double for that reason.

Row lengths: the device filters take 64 samples per lane and 4096 per lane-group
(csrc/srmr.hpp), so 50 and 63 lie below one chunk, 4096 / 4097 at the end of a lane-group, 9001
in the third; 4099 and 8191 are primes for the FFT.
"""
import numpy as np
import pytest

import oracle_srmr as osr

pytestmark = pytest.mark.gpu

RTOL = 1e-9
CASES = osr.cases()


def _torch():
    import torch
    return torch


def dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


@pytest.fixture(scope='module')
def golden():
    with np.load(osr.GOLDEN) as data:
        return {key: data[key] for key in data.files}


def check_values(got, want, what):
    got, want = host(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape)
    error = np.max(np.abs(got - want) / np.abs(want)) if want.size else 0.0
    print(f'{what}: largest relative difference {error:.3e}')
    assert error <= RTOL, (what, error)


def check_bands(got, want, what):
    """got, want (n, ..., N): per channel, within 1e-9 of the channel's peak"""
    got, want = host(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape)
    n = want.shape[0]
    peak = np.abs(want).reshape(n, -1).max(axis=1)
    error = np.max(np.abs(got - want).reshape(n, -1).max(axis=1) / peak)
    print(f'{what}: largest difference {error:.3e} of the peak')
    assert error <= RTOL, (what, error)


# ---- SRMR values ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_srmr_against_reference(name, golden):
    from pb_bss_amd.evaluation import module_srmr, srmr
    case = CASES[name]
    x = dev(case['signal'])
    got = srmr(x, case['sample_rate'], case['n'], case['low_freq'])
    assert got.is_cuda and got.dtype == _torch().float64
    check_values(got, golden[name + '/srmr'], name)
    rows = x.reshape(-1, x.shape[-1])
    _, kept = module_srmr.vad_rows(rows, case['sample_rate'])
    assert host(kept).tolist() == golden[name + '/kept'].tolist(), name


def test_single_row_function_and_numpy_in(golden):
    from pb_bss_amd.evaluation import module_srmr, srmr
    case = CASES['batch_gaps']
    got = srmr(list(case['signal']), case['sample_rate'])  # a list of rows: one batched call
    assert isinstance(got, np.ndarray)
    check_values(got, golden['batch_gaps/srmr'], 'list of rows')
    one = module_srmr.SRMR(case['signal'][1], sample_rate=16000, n=23, low_freq=125)
    assert isinstance(one, np.float64)
    check_values(one, golden['batch_gaps/srmr'][1], 'SRMR of one row')
    got = srmr(dev(case['signal'][:1]))  # rows = 1
    assert tuple(got.shape) == (1,)
    check_values(got, golden['batch_gaps/srmr'][:1], 'one row with a leading axis')


def test_non_contiguous_view(golden):
    from pb_bss_amd.evaluation import srmr
    signal = CASES['batch_gaps']['signal']
    interleaved = np.zeros((3, 2 * signal.shape[1]))
    interleaved[:, ::2] = signal
    view = dev(interleaved)[:, ::2]
    assert not view.is_contiguous()
    check_values(srmr(view), golden['batch_gaps/srmr'], 'strided view')
    check_values(srmr(dev(signal.T.copy()).T), golden['batch_gaps/srmr'], 'transposed view')


def test_all_zero_row_leaves_the_others(golden):
    from pb_bss_amd.evaluation import srmr
    signal = CASES['batch_gaps']['signal']
    batch = np.concatenate([signal[:1], np.zeros((1, signal.shape[1])), signal[1:]])
    got = host(srmr(dev(batch)))
    assert np.isnan(got[1]), got
    check_values(got[[0, 2, 3]], golden['batch_gaps/srmr'], 'rows beside an all-zero row')


def test_doctest_pin():
    from pb_bss_amd.evaluation import srmr
    got = host(srmr(dev(np.stack([osr.doctest_signal()] * 2)), osr.DOCTEST_RATE))
    assert got.shape == (2,) and np.all(np.abs(got - osr.DOCTEST_VALUE) <= 5e-5), got


def test_device_tensor_on_the_current_stream(golden):
    from pb_bss_amd.evaluation import srmr
    torch = _torch()
    case = CASES['one_group_plus_one']
    host_signal = torch.from_numpy(case['signal']).pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = host_signal.to('cuda', non_blocking=True).clone()  # produced on the side stream only
        got = srmr(x)
        assert got.is_cuda and got.device == x.device
    side.synchronize()
    check_values(got, golden['one_group_plus_one/srmr'], 'side stream')


# ---- filterbank ---------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [50, 63, 64, 4096, 4097, 9001, 4099, 8191])
def test_filterbank_row_lengths(N):
    from pb_bss_amd.transform import gammatone_filterbank
    x = osr.speechlike(100 + N, N)
    got = gammatone_filterbank(dev(x))
    assert got.is_cuda and tuple(got.shape) == (23, N)
    check_bands(got, osr.gammatone_filterbank(x), f'N={N}')


@pytest.mark.parametrize('sample_rate,n,low,high', [(16000, 1, 125, 0), (16000, 64, 125, 0),
                                                    (8000, 23, 125, 0), (16000, 23, 300, 5000),
                                                    (8000, 7, 80, 3000.0)])
def test_filterbank_parameters(sample_rate, n, low, high):
    from pb_bss_amd.transform import gammatone_filterbank
    x = osr.speechlike(7, 4300, sample_rate)
    got = gammatone_filterbank(dev(x), sample_rate, n, low, high)
    check_bands(got, osr.gammatone_filterbank(x, sample_rate, n, low, high),
                f'rate={sample_rate} n={n} low={low} high={high}')


def test_filterbank_shapes_and_types(golden):
    from pb_bss_amd.transform import gammatone_filterbank
    x = np.stack([osr.speechlike(60 + r, 4200) for r in range(6)]).reshape(2, 3, 4200)
    want = osr.gammatone_filterbank(x)
    got = gammatone_filterbank(dev(x))
    assert tuple(got.shape) == (23, 2, 3, 4200)
    check_bands(got, want, 'shape (2, 3, N)')
    as_list = gammatone_filterbank(x)  # NumPy in: a list of n arrays, as the reference returns
    assert isinstance(as_list, list) and len(as_list) == 23
    assert all(isinstance(y, np.ndarray) and y.shape == x.shape for y in as_list)
    check_bands(np.stack(as_list), want, 'numpy in')
    x32 = x.astype(np.float32)
    check_bands(gammatone_filterbank(dev(x32)), osr.gammatone_filterbank(x32.astype(np.float64)),
                'float32 rows')
    wide = np.zeros((2, 3, 8400))
    wide[..., ::2] = x
    view = dev(wide)[..., ::2]
    assert not view.is_contiguous()
    check_bands(gammatone_filterbank(view), want, 'strided view')
    for name in ('filterbank_a', 'filterbank_b'):
        sample_rate, n, low, high = golden[name + '/args']
        got = gammatone_filterbank(dev(golden[name + '/input']), int(sample_rate), int(n), low, high)
        check_bands(got, golden[name + '/output'], name)


# ---- the C ABI refuses misuse before it launches anything ------------------------------------------
def test_c_abi_misuse():
    from pb_bss_amd import _lib
    torch = _torch()
    lib, h = _lib.load(), _lib.handle()
    N = 256
    x = torch.zeros((2, N), dtype=torch.float64, device='cuda')
    out = torch.full((2, N), 7.0, dtype=torch.float64, device='cuda')
    lengths = torch.full((2,), -5, dtype=torch.int32, device='cuda')
    bands = torch.full((64, 2, N), 7.0, dtype=torch.float64, device='cuda')
    analytic = torch.zeros((64, 2, N), dtype=torch.complex128, device='cuda')
    coef = torch.zeros((64 * 20,), dtype=torch.float64, device='cuda')
    means = torch.full((2, 64, 8), 7.0, dtype=torch.float64, device='cuda')
    score = torch.full((2,), 7.0, dtype=torch.float64, device='cuda')
    p, s = _lib.ptr, _lib.stream_ptr()
    INVALID, UNSUPPORTED = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED

    def vad(x_=x, rows=2, N_=N, rate=16000, out_=out, lengths_=lengths, h_=h):
        return lib.pbbss_srmr_vad(h_, p(x_), 1, rows, N_, rate, p(out_), p(lengths_), s)

    def filterbank(x_=x, rows=2, N_=N, n=23, coef_=coef, out_=bands, h_=h):
        return lib.pbbss_gammatone(h_, p(x_), 1, rows, N_, None, n, p(coef_), p(out_), s)

    def energies(a_=analytic, rows=2, N_=N, n=23, rate=16000, coef_=coef, out_=means):
        return lib.pbbss_srmr_energies(h, p(a_), rows, N_, p(lengths), n, rate, p(coef_), p(out_),
                                       s)

    def tail(means_=means, rows=2, n=23, erbs=coef, cutoffs=coef, out_=score):
        return lib.pbbss_srmr_score(h, p(means_), rows, n, p(erbs), p(cutoffs), p(out_), s)

    assert vad(h_=None) == INVALID and vad(x_=None) == INVALID and vad(out_=None) == INVALID
    assert vad(lengths_=None) == INVALID and vad(rows=0) == INVALID and vad(N_=0) == INVALID
    assert vad(N_=-1) == INVALID
    assert vad(rate=999) == UNSUPPORTED and vad(N_=(1 << 24) + 1) == UNSUPPORTED
    assert filterbank(h_=None) == INVALID and filterbank(x_=None) == INVALID
    assert filterbank(coef_=None) == INVALID and filterbank(out_=None) == INVALID
    assert filterbank(rows=0) == INVALID and filterbank(N_=0) == INVALID
    assert filterbank(n=0) == UNSUPPORTED and filterbank(n=65) == UNSUPPORTED
    assert filterbank(N_=(1 << 24) + 1) == UNSUPPORTED
    assert energies(a_=None) == INVALID and energies(coef_=None) == INVALID
    assert energies(out_=None) == INVALID and energies(rows=-1) == INVALID
    assert energies(n=65) == UNSUPPORTED and energies(rate=500) == UNSUPPORTED
    assert energies(N_=(1 << 24) + 1) == UNSUPPORTED
    assert tail(means_=None) == INVALID and tail(erbs=None) == INVALID
    assert tail(cutoffs=None) == INVALID and tail(out_=None) == INVALID and tail(rows=0) == INVALID
    assert tail(n=0) == UNSUPPORTED and tail(n=65) == UNSUPPORTED
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    for buffer, fill in ((out, 7.0), (bands, 7.0), (means, 7.0), (score, 7.0), (lengths, -5)):
        assert bool((buffer == fill).all())
    with pytest.raises(NotImplementedError):
        _lib.check(UNSUPPORTED, 'srmr')
