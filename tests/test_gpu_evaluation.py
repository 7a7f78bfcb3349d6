"""GPU: pb_bss_amd.evaluation (si_sdr, get_snr / set_snr, input_sxr, output_sxr) against the
float64 restatement of the reference (tests/oracle_evaluation.py).

Tolerance: the compared quantities are 10 log10 of a ratio of two sums of N non-negative
float64 terms.  In any summation order each sum is within (N - 1) 2^-53 relative (1.5e-11 for
N <= 2^17), the ratio within 3e-11 and the dB value within 1.3e-10; an error of the optimal
scaling enters the residual energy in second order only.  Asserted: 1e-9 dB for every finite
result with |value| <= 60 dB; float32 input is compared with the restatement fed .astype(float64).
"""
import ctypes

import numpy as np
import pytest

import oracle_evaluation as oe

pytestmark = pytest.mark.gpu

TOL = 1e-9
DOC_VALUES = [np.inf, np.inf, -25.127672346460717, 0.481070445785553, 6.3704606032577304,
              6.3704606032577304]


def _torch():
    import torch
    return torch


def dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def wide(x):
    x = np.asarray(x)
    return x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)


def check(got, want, tol=TOL, what=''):
    got, want = host(got), np.asarray(want)
    assert got.dtype == np.float64, got.dtype
    assert got.shape == want.shape, (what, got.shape, want.shape)
    finite = np.isfinite(want)
    np.testing.assert_array_equal(got[~finite], want[~finite])
    if tol == TOL:
        assert np.all(np.abs(want[finite]) <= 60), what  # the range the bound is derived for
    if finite.any():
        worst = np.abs(got[finite] - want[finite]).max()
        print(f'{what}: largest difference {worst:.3e} dB')
        assert worst <= tol, (what, worst)


def span():
    from pb_bss_amd.evaluation import module_si_sdr
    return module_si_sdr.SPAN


ROW_LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 65537]


def row_lengths():
    # the spans cannot be named before the package is imported: resolved inside the test
    return ROW_LENGTHS + ['span-1', 'span', 'span+1', '2*span+1']


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('length', row_lengths())
def test_si_sdr_rowwise(length, dtype):
    from pb_bss_amd.evaluation import si_sdr
    if isinstance(length, str):
        s = span()
        length = {'span-1': s - 1, 'span': s, 'span+1': s + 1, '2*span+1': 2 * s + 1}[length]
    for rows in (1, 5):
        r, e = oe.gen_si_sdr(length + rows, (rows, length), dtype=dtype)
        want = oe.si_sdr(wide(r), wide(e))
        if length == 1:
            # one sample: the estimate is a multiple of the reference and the residual is the
            # rounding error of alpha * r, or zero -- far beyond 60 dB either way
            got = host(si_sdr(dev(r), dev(e)))
            assert got.shape == (rows,) and np.all(got > 250) and np.all(want > 250), (got, want)
            continue
        check(si_sdr(dev(r), dev(e)), want, what=f'rowwise N={length} rows={rows}')
        if dtype == np.float64:
            check(si_sdr(r, e), want, what=f'rowwise numpy N={length} rows={rows}')
            check(si_sdr(dev(r[0]), dev(e[0])), want[0], what='one row')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_si_sdr_outer(dtype):
    from pb_bss_amd.evaluation import si_sdr
    N = 1000
    r, _ = oe.gen_si_sdr(0, (3, 2, N), dtype=dtype)
    mix = oe.gen_signals(1, (3, 3, 2), np.float64)
    e = (np.einsum('bek,bkn->ben', mix, wide(r)) + 0.1 * oe.gen_signals(2, (3, 3, N))).astype(dtype)
    want = oe.si_sdr(wide(r)[:, :, None], wide(e)[:, None])
    assert want.shape == (3, 2, 3)
    check(si_sdr(dev(r)[:, :, None], dev(e)[:, None]), want, what='outer')
    check(si_sdr(dev(r)[:, None], dev(e)[:, :, None]), want.transpose(0, 2, 1),
          what='outer transposed')
    # a reference that all batch items share
    e0 = (np.einsum('bek,kn->ben', mix, wide(r[0])) + 0.1 * oe.gen_signals(2, (3, 3, N))).astype(dtype)
    check(si_sdr(dev(r[0])[:, None], dev(e0)[:, None]),
          oe.si_sdr(wide(r[0])[:, None], wide(e0)[:, None]), what='outer, shared reference')
    # broadcast shapes beside the two forms
    a = oe.gen_signals(3, (2, 1, 3, N), dtype)
    b = (oe.gen_signals(4, (1, 4, 1, N)) + 0.5 * wide(a).sum(2, keepdims=True)[:1]).astype(dtype)
    check(si_sdr(dev(a), dev(b)), oe.si_sdr(wide(a), wide(b)), what='(2,1,3,N) x (1,4,1,N)')
    a = oe.gen_signals(5, (2, 1, 3, 1, 257), dtype)
    b = (oe.gen_signals(6, (1, 4, 1, 2, 257)) + 0.5 * wide(a).sum((0, 2), keepdims=True)).astype(dtype)
    want = oe.si_sdr(wide(a), wide(b))
    assert want.shape == (2, 4, 3, 2)
    check(si_sdr(dev(a), dev(b)), want, what='copy path')
    # more rows than a lane keeps: the copy path
    a = oe.gen_signals(7, (9, 1, 300), dtype)
    b = (oe.gen_signals(8, (1, 2, 300)) + 0.3 * wide(a).sum(0, keepdims=True)).astype(dtype)
    check(si_sdr(dev(a), dev(b)), oe.si_sdr(wide(a), wide(b)), what='nine reference rows')


def test_si_sdr_docstring_cases():
    from pb_bss_amd.evaluation import si_sdr
    np.random.seed(0)
    reference = np.random.randn(100)
    pairs = [(reference, reference), (reference, reference * 2), (reference, np.flip(reference)),
             (reference, reference + np.flip(reference)), (reference, reference + 0.5),
             (reference, reference * 2 + 1)]
    got = np.array([si_sdr(r, e) for r, e in pairs])
    assert np.isposinf(got[0]) and np.isposinf(got[1]), got
    check(got, np.array(DOC_VALUES), what='docstring')
    assert np.isnan(si_sdr([1., 0], [0., 0]))  # never predict only zeros
    assert np.isnan(si_sdr([0., 0], [1., 0]))  # a zero reference
    two = si_sdr([reference, reference], [reference * 2 + 1, reference * 1 + 0.5])
    check(two, np.array([6.3704606032577304, 6.3704606032577304]), what='two rows')
    # power-of-two multiples stay exact across several spans and in float32
    long = dev(oe.gen_signals(0, (2, 2 * span() + 1), np.float32))
    assert np.isposinf(host(si_sdr(long, long * 0.25))).all()
    assert np.isposinf(host(si_sdr(long[:, None], long[:, None] * 4.0))).all()


@pytest.mark.parametrize('length', [4097, 131072])
def test_si_sdr_high_sdr(length):
    """about 117 dB: explicit residuals land near 1e-11 dB, the one-pass form
    sum e^2 - alpha^2 sum r^2 misses by 2e-4 dB and more"""
    from pb_bss_amd.evaluation import si_sdr
    r = oe.gen_signals(0, (2, length))
    e = 0.7 * r + 1e-6 * oe.gen_signals(1, (2, length))
    want = oe.si_sdr(r, e)
    assert np.all((want > 110) & (want < 125)), want
    check(si_sdr(dev(r), dev(e)), want, tol=1e-6, what=f'high SDR N={length}')


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_si_sdr_alignment_and_strides(dtype):
    from pb_bss_amd.evaluation import si_sdr
    for length in (1003, 1000):  # row pitch 1004: rows share their alignment; 1001: they do not
        r, e = oe.gen_si_sdr(length, (5, length + 1), dtype=dtype)
        # every estimate holds a share of every reference: the cross pairs stay above -60 dB
        e = (wide(e) + 0.5 * wide(r).sum(0, keepdims=True)).astype(dtype)
        rd, ed = dev(r)[:, 1:], dev(e)[:, 1:]
        assert rd.data_ptr() % 16 != 0 and not rd.is_contiguous()
        plain = si_sdr(rd.contiguous(), ed.contiguous())
        check(plain, oe.si_sdr(wide(r)[:, 1:], wide(e)[:, 1:]), what=f'contiguous N={length}')
        check(si_sdr(rd, ed), host(plain), what=f'odd offset N={length}')
        check(si_sdr(rd, ed.contiguous()), host(plain), what=f'mixed alignment N={length}')
        check(si_sdr(rd[:, None], ed[None]), oe.si_sdr(wide(r)[:, None, 1:], wide(e)[None, :, 1:]),
              what=f'odd offset, outer N={length}')
    r, e = oe.gen_si_sdr(9, (3, 5, 600), dtype=dtype)
    rp, ep = dev(r).permute(1, 0, 2), dev(e).permute(1, 0, 2)
    assert not rp.is_contiguous()
    plain = si_sdr(rp.contiguous(), ep.contiguous())
    check(plain, oe.si_sdr(wide(r), wide(e)).T, what='permuted, contiguous')
    check(si_sdr(rp, ep), host(plain), what='permuted batch axis')
    # a sample axis with a stride
    check(si_sdr(dev(r)[..., ::2], dev(e)[..., ::2]), oe.si_sdr(wide(r)[..., ::2], wide(e)[..., ::2]),
          what='strided samples')


OUTPUT_SHAPES = [(2, 3), (3, 3), (1, 1), (1, 2), (4, 5)]


@pytest.mark.parametrize('dtype', [np.float32, np.float64, np.complex64])
@pytest.mark.parametrize('Ks,Kt', OUTPUT_SHAPES)
def test_output_sxr(Ks, Kt, dtype):
    from pb_bss_amd.evaluation.sxr_module import output_sxr
    co, no = oe.gen_output_case(10 * Ks + Kt, (5,), Ks, Kt, 1000, dtype)
    for average in (True, False):
        details = {}
        want, want_sel = oe.output_sxr(wide(co), wide(no), average, details)
        assert details['margin'].min() >= oe.MARGIN  # the best selection is well determined
        if Kt > 1:
            assert len({tuple(s) for s in want_sel.tolist()}) > 1  # the items pick differently
        got, sel = output_sxr(dev(co), dev(no), average, return_selection=True)
        assert type(got).__name__ == 'SXR' and got._fields == ('sdr', 'sir', 'snr')
        np.testing.assert_array_equal(host(sel), want_sel)
        assert host(sel).dtype == np.int64
        for name in got._fields:
            if name == 'sir' and Ks == 1:
                assert np.isposinf(host(getattr(got, name))).all()
            check(getattr(got, name), getattr(want, name), what=f'output {name} {Ks},{Kt}')
    # one item, no batch axis, NumPy in
    one, sel = output_sxr(co[2], no[2], False, return_selection=True)
    np.testing.assert_array_equal(sel, want_sel[2])
    assert isinstance(one.sdr, np.ndarray) and one.sdr.shape == (Ks,)
    check(one.sdr, want.sdr[2], what='one item')


def test_output_sxr_return_forms():
    from pb_bss_amd.evaluation.sxr_module import output_sxr
    co, no = oe.gen_output_case(1, (), 2, 3, 1000)
    for average in (True, False):
        want, _ = oe.output_sxr(co, no, average)
        as_tuple = output_sxr(co, no, average, False)
        as_dict = output_sxr(co, no, average_sources=average, return_dict=True)
        assert isinstance(as_tuple, tuple) and sorted(as_dict) == ['sdr', 'sir', 'snr']
        for name in ('sdr', 'sir', 'snr'):
            check(getattr(as_tuple, name), getattr(want, name), what=f'tuple {name}')
            check(as_dict[name], getattr(want, name), what=f'dict {name}')
    # as in the reference, a str prefix returns the tuple
    assert isinstance(output_sxr(co, no, True, 'out_'), tuple)
    with_sel = output_sxr(co, no, return_dict=True, return_selection=True)
    assert isinstance(with_sel[0], dict) and with_sel[1].shape == (2,)


@pytest.mark.parametrize('Ks,Kt', [(3, 3), (2, 3)])
def test_output_sxr_exact_tie(Ks, Kt):
    """every contribution is the same signal: all totals are bit-equal, the first selection wins"""
    from pb_bss_amd.evaluation.sxr_module import output_sxr
    x = oe.gen_signals(0, (1000,))
    co = np.ascontiguousarray(np.broadcast_to(x, (4, Ks, Kt, 1000)))
    no = 0.1 * oe.gen_signals(1, (4, Kt, 1000))
    got, sel = output_sxr(dev(co), dev(no), False, return_selection=True)
    np.testing.assert_array_equal(host(sel), np.tile(np.arange(Ks), (4, 1)))
    want, want_sel = oe.output_sxr(co, no, False)
    np.testing.assert_array_equal(want_sel, host(sel))
    check(got.sdr, want.sdr, what='tie sdr')


def test_output_sxr_bounds():
    from pb_bss_amd.evaluation.sxr_module import output_sxr
    z = _torch().zeros
    with pytest.raises(NotImplementedError, match='at most 8'):
        output_sxr(z((2, 9, 10), device='cuda'), z((9, 10), device='cuda'))
    with pytest.raises(AssertionError):
        output_sxr(z((3, 2, 10), device='cuda'), z((2, 10), device='cuda'))
    # the largest served case: 8! selections
    co, no = oe.gen_output_case(3, (2,), 8, 8, 64)
    details = {}
    want, want_sel = oe.output_sxr(co, no, True, details)
    assert details['margin'].min() >= oe.MARGIN
    got, sel = output_sxr(dev(co), dev(no), True, return_selection=True)
    np.testing.assert_array_equal(host(sel), want_sel)
    check(got.sdr, want.sdr, what='8 x 8')


@pytest.mark.parametrize('dtype', [np.float32, np.float64, np.complex64])
def test_input_sxr(dtype):
    from pb_bss_amd.evaluation.sxr_module import input_sxr
    im, no = oe.gen_input_case(0, (3,), 3, 4, 1000, dtype)
    for sources in (True, False):
        for channels in (True, False):
            want = oe.input_sxr(wide(im), wide(no), sources, channels)
            got = input_sxr(dev(im), dev(no), sources, channels)
            assert type(got).__name__ == 'SXR'
            for name in got._fields:
                check(getattr(got, name), getattr(want, name),
                      what=f'input {name} {sources} {channels}')
            one = input_sxr(im[1], no[1], sources, channels, return_dict='in_')
            assert sorted(one) == ['in_sdr', 'in_sir', 'in_snr']
            check(one['in_sdr'], want.sdr[1], what='one item')
    assert sorted(input_sxr(im[0], no[0], return_dict=True)) == ['sdr', 'sir', 'snr']
    with pytest.raises(TypeError):
        input_sxr(im[0], no[0], return_dict=3)
    im, no = oe.gen_input_case(1, (), 1, 2, 1000, dtype)
    got = input_sxr(dev(im), dev(no), False, False)
    assert np.isposinf(host(got.sir)).all() and host(got.sir).shape == (1, 2)
    check(got.snr, oe.input_sxr(wide(im), wide(no), False, False).snr, what='K=1 snr')
    im, no = oe.gen_input_case(2, (), 9, 29, 100, dtype)  # the reference's largest shape
    for sources in (True, False):
        for channels in (True, False):
            want = oe.input_sxr(wide(im), wide(no), sources, channels)
            check(input_sxr(dev(im), dev(no), sources, channels).sdr, want.sdr, what='K=9 D=29')


def test_get_snr_and_set_snr():
    from pb_bss_amd.evaluation.sxr_module import get_snr, set_snr
    assert get_snr([1, 2, 3], [1, 2, 3]) == 0.0
    for dtype in (np.float32, np.float64, np.complex64, np.complex128):
        X = oe.gen_signals(0, (3, 4, 1000), dtype)
        N = (0.3 * oe.gen_signals(1, (3, 4, 1000), dtype)).astype(dtype)
        for kwargs in ({}, {'axis': -1}, {'axis': 0}, {'axis': (0, 2)},
                       {'axis': 1, 'keepdims': True}, {'axis': None, 'keepdims': True}):
            want = oe.get_snr(wide(X), wide(N), **kwargs)
            check(get_snr(dev(X), dev(N), **kwargs), want, what=f'get_snr {dtype.__name__} {kwargs}')
        check(get_snr(X, N, axis=-1), oe.get_snr(wide(X), wide(N), axis=-1), what='get_snr numpy')
    X = oe.gen_signals(2, (2, 4, 1000))
    N = oe.gen_signals(3, (2, 4, 1000))
    # in place, NumPy and tensor
    Nn = N.copy()
    assert set_snr(X, Nn, 5.0) is None
    check(get_snr(X, Nn), np.float64(5.0), what='set_snr numpy')
    np.testing.assert_allclose(Nn, N * 10 ** (-(5.0 - oe.get_snr(X, N)) / 20), rtol=1e-12)
    Nd = dev(N)
    set_snr(dev(X), Nd, np.array([[[5.0]], [[-3.0]]]), axis=(1, 2))
    check(get_snr(dev(X), Nd, axis=(1, 2)), np.array([5.0, -3.0]), what='set_snr tensor')
    # not in place
    Nd = dev(N)
    Xo, No = set_snr(dev(X), Nd, 12.0, inplace=False)
    np.testing.assert_array_equal(host(Nd), N)
    np.testing.assert_array_equal(host(Xo), X)
    check(get_snr(Xo, No), np.float64(12.0), what='set_snr copy')
    Xo, No = set_snr(X, N, 12.0, current_snr=0.0, inplace=False)
    np.testing.assert_allclose(No, N * 10 ** (-12.0 / 20), rtol=1e-15)


def test_determinism():
    from pb_bss_amd.evaluation import si_sdr
    from pb_bss_amd.evaluation.sxr_module import input_sxr, output_sxr
    torch = _torch()
    r, e = (dev(x) for x in oe.gen_si_sdr(0, (3, 65537), dtype=np.float32))
    assert torch.equal(si_sdr(r, e), si_sdr(r, e))
    assert torch.equal(si_sdr(r[:, None], e[None]), si_sdr(r[:, None], e[None]))
    co, no = (dev(x) for x in oe.gen_output_case(0, (4,), 3, 4, 10000, np.float32))
    a, b = output_sxr(co, no, False), output_sxr(co, no, False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    im, no = (dev(x) for x in oe.gen_input_case(0, (4,), 3, 4, 10000, np.complex64))
    a, b = input_sxr(im, no, False, False), input_sxr(im, no, False, False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_placement():
    from pb_bss_amd.evaluation import si_sdr
    from pb_bss_amd.evaluation.sxr_module import get_snr, input_sxr, output_sxr
    torch = _torch()
    r, e = oe.gen_si_sdr(0, (3, 500))
    co, no = oe.gen_output_case(0, (2,), 2, 3, 500)
    im, ni = oe.gen_input_case(0, (2,), 2, 3, 500)
    results = [si_sdr(r, e), get_snr(r, e, axis=-1), *output_sxr(co, no), *input_sxr(im, ni),
               *output_sxr(co, no, return_selection=True)[1:]]
    for x in results:
        assert isinstance(x, np.ndarray), type(x)
    assert all(x.dtype == np.float64 for x in results[:-1]) and results[-1].dtype == np.int64
    assert isinstance(si_sdr(r[0], e[0]), np.float64)
    for dtype in (torch.float32, torch.float64):
        d = [dev(x).to(dtype) for x in (r, e, co, no, im, ni)]
        results = [si_sdr(d[0], d[1]), get_snr(d[0], d[1], axis=-1), *output_sxr(d[2], d[3]),
                   *input_sxr(d[4], d[5])]
        for x in results:
            assert isinstance(x, torch.Tensor) and x.device == d[0].device, x
            assert x.dtype == torch.float64
        assert output_sxr(d[2], d[3], return_selection=True)[1].device == d[0].device
    # a host tensor in: a host tensor out
    out = si_sdr(torch.from_numpy(r), torch.from_numpy(e))
    assert isinstance(out, torch.Tensor) and out.device.type == 'cpu'
    check(out, oe.si_sdr(r, e), what='host tensor')


def test_raw_c_abi_errors():
    torch = _torch()
    from pb_bss_amd import _lib
    lib = _lib.load()
    h, stream = _lib.handle(0), _lib.stream_ptr(0)
    N = 100
    x = torch.zeros((2, 9, 9, N), dtype=torch.float32, device='cuda')
    out = torch.zeros((2 * 3 * 81,), dtype=torch.float64, device='cuda')
    sel = torch.zeros((2 * 9,), dtype=torch.int64, device='cuda')
    X, O, S = _lib.ptr(x), _lib.ptr(out), _lib.ptr(sel)

    def power(handle=h, xx=X, oo=O, dtype=0, rows=4, length=N):
        return lib.pbbss_signal_power(handle, xx, dtype, rows, length, N, oo, stream)
    assert power() == _lib.OK
    assert power(handle=None) == power(xx=None) == power(oo=None) == _lib.ERR_INVALID_ARG
    assert power(dtype=4) == power(rows=0) == power(length=0) == _lib.ERR_INVALID_ARG
    # a pointer that is no multiple of the element size, and a grid beyond 2^24 - 1 workgroups
    odd = ctypes.c_void_p(x.data_ptr() + 2)
    half = ctypes.c_void_p(x.data_ptr() + 4)
    assert power(xx=odd) == power(xx=half, dtype=1) == power(xx=half, dtype=3) \
        == _lib.ERR_INVALID_ARG
    assert power(xx=half, rows=2) == _lib.OK
    assert power(rows=1 << 24, length=1) == _lib.ERR_UNSUPPORTED

    def sisdr(handle=h, rr=X, ee=X, oo=O, Kr=2, Ke=3, length=N):
        return lib.pbbss_si_sdr(handle, rr, ee, 0, 2, Kr, Ke, length, 9 * N, N, 9 * N, N, oo, stream)
    assert sisdr() == _lib.OK
    assert sisdr(handle=None) == sisdr(rr=None) == sisdr(ee=None) == sisdr(oo=None) \
        == _lib.ERR_INVALID_ARG
    assert sisdr(Kr=0) == sisdr(length=0) == _lib.ERR_INVALID_ARG
    assert sisdr(Kr=9) == sisdr(Ke=9) == _lib.ERR_UNSUPPORTED
    assert sisdr(rr=odd) == sisdr(ee=odd) == _lib.ERR_INVALID_ARG

    def output(handle=h, cc=X, nn=X, oo=O, ss=S, mm=O, Ks=2, Kt=3, average=1):
        return lib.pbbss_output_sxr(handle, cc, nn, 0, 2, Ks, Kt, N, average, oo, ss, mm, stream)
    assert output() == _lib.OK
    assert output(handle=None) == output(cc=None) == output(nn=None) == output(oo=None) \
        == output(ss=None) == output(mm=None) == _lib.ERR_INVALID_ARG
    assert output(mm=None, average=0) == _lib.OK
    assert output(Ks=4, Kt=3) == _lib.ERR_INVALID_ARG
    assert output(Kt=9) == output(Ks=9, Kt=9) == _lib.ERR_UNSUPPORTED
    assert output(cc=odd) == output(nn=odd) == _lib.ERR_INVALID_ARG

    def inputs(handle=h, ii=X, nn=X, oo=O, K=3, D=4):
        return lib.pbbss_input_sxr(handle, ii, nn, 0, 2, K, D, N, 0, 0, oo, stream)
    assert inputs() == _lib.OK
    assert inputs(handle=None) == inputs(ii=None) == inputs(nn=None) == inputs(oo=None) \
        == _lib.ERR_INVALID_ARG
    assert inputs(K=0) == _lib.ERR_INVALID_ARG
    assert inputs(K=10) == inputs(D=30) == _lib.ERR_UNSUPPORTED
    assert inputs(ii=odd) == inputs(nn=odd) == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
