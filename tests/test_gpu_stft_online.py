"""Streaming STFT / inverse STFT (pb_bss_amd.transform.OnlineSTFT / OnlineISTFT, kernels
csrc/stft_stream.hip) on the device: bit-identity with the offline transforms under every blocking
of tests/oracle_stft_online.py, agreement with the NumPy restatement within the bounds of
tests/test_gpu_stft.py (its assert_allclose calls as they stand: atol 1e-11 for complex128 frames
of unit-variance noise, 2e-5 for complex64, 1e-12 for the inverse, each with numpy's default
rtol of 1e-7, which is what carries the R = 1 case: the biorthogonal window of a periodic Blackman
window without overlap is 1 / w, up to 1e16), independence of rows, objects and forks, NaN
containment, refusals, and independence of what ran before on the same handle.

The shapes are the smallest at which the kernels can go wrong (oracle_stft_online.CASES)."""
import ctypes

import numpy as np
import pytest

import oracle_stft_online as so

pytestmark = pytest.mark.gpu

FWD_ATOL = {np.complex128: 1e-11, np.complex64: 2e-5}   # tests/test_gpu_stft.py
INV_ATOL = 1e-12                                        # tests/test_gpu_stft.py


def _samples(channels, n, seed):
    """Unit-variance noise that float32 holds exactly: the float32 and float64 streams agree."""
    x = np.random.default_rng(seed).standard_normal((channels, n)).astype(np.float32)
    return x


def _spectra(lead, T, F, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(lead + (T, F)) + 1j * rng.standard_normal(lead + (T, F))


def _forward(stream, x, lengths, pad=True, dtypes=None):
    """Concatenation (frame axis 1 in both layouts) of every step_block and of flush."""
    import torch
    parts = []
    for i, block in enumerate(so.split(x, lengths)):
        if dtypes is not None:
            block = block.to(dtypes[i % len(dtypes)])
        parts.append(stream.step_block(block))
    counts = [int(p.shape[1]) for p in parts]
    parts.append(stream.flush(pad))
    return torch.cat(parts, dim=1), counts


def _inverse(stream, X, lengths, axis=-2):
    import torch
    parts = [stream.step_block(b) for b in so.split(X, lengths, axis=axis)]
    parts.append(stream.flush())
    return torch.cat(parts, dim=-1)


@pytest.mark.parametrize('channels', [1, 3])
@pytest.mark.parametrize('fading', [True, False])
@pytest.mark.parametrize('case', so.CASES, ids=so.CASE_IDS)
def test_streaming_forward_is_the_offline_stft(case, fading, channels):
    import torch
    from pb_bss_amd.transform import OnlineSTFT, stft
    size, shift, wl, n = case
    x32 = torch.from_numpy(_samples(channels, n, seed=size + channels)).cuda()
    blockings = so.blockings(n, shift, wl, size)
    combo = 0
    for in_dtype in (torch.float32, torch.float64):
        for out_dtype in (np.complex128, np.complex64):
            for layout in ('f t d', None):
                pad = combo % 2 == 0
                combo += 1
                x = x32.to(in_dtype)
                ref = stft(x, size, shift, window_length=wl, fading=fading, pad=pad,
                           layout=layout, dtype=out_dtype)
                stream = OnlineSTFT(channels, size, shift, window_length=wl, fading=fading,
                                    layout=layout, dtype=out_dtype)   # reused: flush resets it
                for name, lengths in blockings.items():
                    if name == 'ones' and combo not in (1, 8):
                        continue
                    got, counts = _forward(stream, x, lengths, pad)
                    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.shape)
                    assert torch.equal(got, ref), (name, in_dtype, out_dtype, layout, pad)
                    assert stream.samples_seen == stream.frames_seen == 0
                    if name == 'short' and shift > 1:
                        assert 0 in counts  # a call that completes no frame
    # float32 and float64 blocks alternate in one stream: the history is float64, widening exact
    stream = OnlineSTFT(channels, size, shift, window_length=wl, fading=fading)
    got, _ = _forward(stream, x32, blockings['irregular'], True,
                      dtypes=(torch.float32, torch.float64))
    assert torch.equal(got, stft(x32, size, shift, window_length=wl, fading=fading,
                                 layout='f t d'))


@pytest.mark.parametrize('rows', [1, 3])
@pytest.mark.parametrize('fading', [True, False])
@pytest.mark.parametrize('case', so.CASES, ids=so.CASE_IDS)
def test_streaming_inverse_is_the_offline_istft(case, fading, rows):
    import torch
    from pb_bss_amd.transform import OnlineISTFT, istft
    size, shift, wl, _ = case
    T, F, R = so.FRAMES, size // 2 + 1, wl // shift
    X128 = torch.from_numpy(_spectra((rows,), T, F, seed=size + rows)).cuda()
    blockings = so.frame_blockings(T, R, size)
    for dtype in (torch.complex128, torch.complex64):
        X = X128.to(dtype)
        ref = istft(X, size, shift, window_length=wl, fading=fading)
        assert ref.shape == (rows, T * shift + (wl - shift) * (-1 if fading else 1))
        for layout in (None, 'f t'):
            stream = OnlineISTFT(size, shift, window_length=wl, fading=fading, layout=layout)
            # 'f t': (rows, F, T) cut along the last axis: strided views, read in place
            src, axis = (X, -2) if layout is None else (X.transpose(-1, -2).contiguous(), -1)
            for name, lengths in blockings.items():
                got = _inverse(stream, src, lengths, axis)
                assert got.dtype == torch.float64 and got.shape == ref.shape, (name, got.shape)
                assert torch.equal(got, ref), (name, dtype, layout)
                assert stream.frames_seen == 0
    # no leading axis at all: one row
    stream = OnlineISTFT(size, shift, window_length=wl, fading=fading)
    got = _inverse(stream, X128[0], blockings['irregular'])
    assert torch.equal(got, istft(X128[0], size, shift, window_length=wl, fading=fading))


@pytest.mark.parametrize('fading', [True, False])
@pytest.mark.parametrize('case', so.CASES, ids=so.CASE_IDS)
def test_streams_agree_with_the_restatement(case, fading):
    """NumPy in, NumPy out, block by block against the step / flush classes of the restatement."""
    from pb_bss_amd.transform import OnlineISTFT, OnlineSTFT
    size, shift, wl, n = case
    x = _samples(3, n, seed=size).astype(np.float64)
    for dtype in (np.complex128, np.complex64):
        dev = OnlineSTFT(3, size, shift, window_length=wl, fading=fading, layout=None, dtype=dtype)
        ref = so.OnlineSTFT(3, size, shift, window_length=wl, fading=fading)
        for block in so.split(x, so.blockings(n, shift, wl, size)['irregular']):
            got, want = dev.step_block(block), ref.step(block)
            assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == want.shape
            np.testing.assert_allclose(got, want, atol=FWD_ATOL[dtype])
        got, want = dev.flush(), ref.flush()
        assert got.shape == want.shape and got.shape[1] > 0
        np.testing.assert_allclose(got, want, atol=FWD_ATOL[dtype])
    X = _spectra((3,), so.FRAMES, size // 2 + 1, seed=size + 1)
    dev = OnlineISTFT(size, shift, window_length=wl, fading=fading)
    ref = so.OnlineISTFT(size, shift, window_length=wl, fading=fading)
    for block in so.split(X, so.frame_blockings(so.FRAMES, wl // shift, size)['irregular'], -2):
        got, want = dev.step_block(block), ref.step(block)
        assert isinstance(got, np.ndarray) and got.shape == want.shape
        np.testing.assert_allclose(got, want, atol=INV_ATOL)
    got, want = dev.flush(), ref.flush()
    assert got.shape == want.shape == (3, 0 if fading else wl - shift)
    np.testing.assert_allclose(got, want, atol=INV_ATOL)


@pytest.mark.parametrize('case', [so.CASES[1], so.CASES[4]], ids=[so.CASE_IDS[1], so.CASE_IDS[4]])
def test_rows_objects_and_forks_are_independent(case):
    import torch
    from pb_bss_amd.transform import OnlineISTFT, OnlineSTFT, istft, stft
    size, shift, wl, n = case
    kw = dict(window_length=wl, fading=True)
    x = torch.from_numpy(_samples(3, n, seed=7)).cuda()
    y = torch.from_numpy(_samples(3, n, seed=8)).cuda()
    lengths = so.blockings(n, shift, wl, size)['irregular']
    # channels together == each channel alone
    together, _ = _forward(OnlineSTFT(3, size, shift, layout=None, **kw), x, lengths)
    for c in range(3):
        alone, _ = _forward(OnlineSTFT(1, size, shift, layout=None, **kw), x[c:c + 1], lengths)
        assert torch.equal(together[c:c + 1], alone), c
    # two objects advanced alternately; a fork in the middle of the stream
    a, b = OnlineSTFT(3, size, shift, **kw), OnlineSTFT(3, size, shift, **kw)
    pa, pb, pf, fork = [], [], [], None
    for i, (ba, bb) in enumerate(zip(so.split(x, lengths), so.split(y, lengths))):
        if i == 4:
            fork = a.clone()
            assert fork.samples_seen == a.samples_seen and fork.frames_seen == a.frames_seen
            assert fork.history.data_ptr() != a.history.data_ptr()
            pf = list(pa)
        pa.append(a.step_block(ba))
        pb.append(b.step_block(bb))
        if fork is not None:
            pf.append(fork.step_block(ba))
    pb.append(b.flush())
    pf.append(fork.flush())
    pa.append(a.flush())
    assert torch.equal(torch.cat(pa, 1), stft(x, size, shift, layout='f t d', **kw))
    assert torch.equal(torch.cat(pb, 1), stft(y, size, shift, layout='f t d', **kw))
    assert torch.equal(torch.cat(pf, 1), torch.cat(pa, 1))
    # the same for the inverse
    T, F, R = so.FRAMES, size // 2 + 1, wl // shift
    X = torch.from_numpy(_spectra((3,), T, F, seed=9)).cuda()
    Z = torch.from_numpy(_spectra((3,), T, F, seed=10)).cuda()
    flengths = so.frame_blockings(T, R, size)['irregular']
    together = _inverse(OnlineISTFT(size, shift, **kw), X, flengths)
    for r in range(3):
        assert torch.equal(together[r:r + 1],
                           _inverse(OnlineISTFT(size, shift, **kw), X[r:r + 1], flengths)), r
    a, b = OnlineISTFT(size, shift, **kw), OnlineISTFT(size, shift, **kw)
    pa, pb, pf, fork = [], [], [], None
    for i, (ba, bb) in enumerate(zip(so.split(X, flengths, -2), so.split(Z, flengths, -2))):
        if i == 4:
            fork = a.clone()
            assert fork.frames_seen == a.frames_seen
            assert fork.tail.data_ptr() != a.tail.data_ptr() or fork.tail.numel() == 0
            pf = list(pa)
        pa.append(a.step_block(ba))
        pb.append(b.step_block(bb))
        if fork is not None:
            pf.append(fork.step_block(ba))
    for parts, obj in ((pa, a), (pb, b), (pf, fork)):
        parts.append(obj.flush())
    assert torch.equal(torch.cat(pa, -1), istft(X, size, shift, **kw))
    assert torch.equal(torch.cat(pb, -1), istft(Z, size, shift, **kw))
    assert torch.equal(torch.cat(pf, -1), torch.cat(pa, -1))


@pytest.mark.parametrize('fading', [True, False])
def test_nan_stays_where_it_is(fading):
    """A NaN sample contaminates exactly the frames that cover it, a NaN frame exactly the hops it
    covers; window_length clean samples (R clean frames) later the output is clean again, and a
    flushed stream carries nothing over."""
    import torch
    from pb_bss_amd.transform import OnlineISTFT, OnlineSTFT, istft, stft
    size, shift, wl, n = so.CASES[3]
    fade = wl - shift if fading else 0
    x = _samples(3, n, seed=3).astype(np.float64)
    clean = torch.from_numpy(x).cuda()
    p = 150
    x[1, p] = np.nan
    stream = OnlineSTFT(3, size, shift, window_length=wl, fading=fading, layout=None)
    lengths = so.blockings(n, shift, wl, size)['short']
    got, _ = _forward(stream, torch.from_numpy(x).cuda(), lengths)
    t = np.arange(got.shape[1])
    covered = (t * shift - fade <= p) & (p < t * shift - fade + wl)
    assert covered.sum() == wl // shift
    bad = torch.isnan(got.real) | torch.isnan(got.imag)
    want = np.zeros((3, got.shape[1], 1), bool)
    want[1, covered] = True
    assert torch.equal(bad, torch.from_numpy(np.broadcast_to(want, bad.shape).copy()).cuda())
    ref = stft(clean, size, shift, window_length=wl, fading=fading)
    assert torch.equal(got[~bad], ref[~bad])            # every clean frame is the clean stream's
    again, _ = _forward(stream, clean, lengths)          # the flushed object: nothing sticks
    assert torch.equal(again, ref)
    # inverse
    T, F, R = so.FRAMES, size // 2 + 1, wl // shift
    X = _spectra((3,), T, F, seed=4)
    Xc = torch.from_numpy(X).cuda()
    t0 = 11
    X[1, t0, 5] = complex(np.nan, 0.0)
    stream = OnlineISTFT(size, shift, window_length=wl, fading=fading)
    flengths = so.frame_blockings(T, R, size)['short']
    got = _inverse(stream, torch.from_numpy(X).cuda(), flengths)
    pos = np.arange(got.shape[-1]) + fade                # position in the uncut signal
    want = np.zeros(tuple(got.shape), bool)
    want[1] = (t0 * shift <= pos) & (pos < t0 * shift + wl)
    assert want[1].sum() == wl
    bad = torch.isnan(got)
    assert torch.equal(bad, torch.from_numpy(want).cuda())
    ref = istft(Xc, size, shift, window_length=wl, fading=fading)
    assert torch.equal(got[~bad], ref[~bad])
    assert torch.equal(_inverse(stream, Xc, flengths), ref)


def test_refusals():
    import torch
    from pb_bss_amd import _lib
    from pb_bss_amd.transform import OnlineISTFT, OnlineSTFT
    with pytest.raises(NotImplementedError):
        OnlineSTFT(2, 500, 125)
    with pytest.raises(NotImplementedError):
        OnlineISTFT(500, 125)
    with pytest.raises(ValueError):
        OnlineISTFT(512, 100)                            # window_length % shift != 0
    with pytest.raises(ValueError):
        OnlineSTFT(2, 512, 128, layout='t f d')
    with pytest.raises(AssertionError):
        OnlineSTFT(2, 64, 16).step_block(torch.zeros(3, 40, device='cuda'))
    with pytest.raises(AssertionError):
        OnlineISTFT(64, 16).step_block(torch.zeros(2, 5, 32, dtype=torch.complex128, device='cuda'))
    inv = OnlineISTFT(64, 16)
    inv.step_block(torch.zeros(2, 5, 33, dtype=torch.complex128, device='cuda'))
    with pytest.raises(AssertionError):                  # the rows are fixed by the first call
        inv.step_block(torch.zeros(3, 5, 33, dtype=torch.complex128, device='cuda'))
    # the C boundary: argument checks only (the two valid calls run on zeros)
    lib, h = _lib.load(), _lib.handle(torch.cuda.current_device())
    dev = dict(device='cuda')
    x = torch.zeros(2, 40, dtype=torch.float64, **dev)
    h0, h1 = torch.zeros(2, 63, dtype=torch.float64, **dev), torch.zeros(2, 63, dtype=torch.float64, **dev)
    w = torch.ones(64, dtype=torch.float64, **dev)
    out = torch.zeros(2, 1, 33, dtype=torch.complex128, **dev)
    P = lambda a: ctypes.c_void_p(a.data_ptr())           # noqa: E731

    def fwd(x=P(x), C=2, n=40, hin=P(h0), hout=P(h1), m=0, window=P(w), o=P(out)):
        return lib.pbbss_stft_stream(h, x, 1, C, n, hin, hout, 0, 0, m, 0, 64, 16, 64, window, 0,
                                     0, 1, o, None)
    assert fwd() == _lib.OK and fwd(n=64, m=1, x=None) == _lib.ERR_INVALID_ARG
    assert fwd(x=None) == _lib.ERR_INVALID_ARG
    assert fwd(hin=None) == _lib.ERR_INVALID_ARG and fwd(hout=None) == _lib.ERR_INVALID_ARG
    assert fwd(hout=P(h0)) == _lib.ERR_INVALID_ARG       # the two histories must differ
    assert fwd(window=None) == _lib.ERR_INVALID_ARG
    assert fwd(n=-1) == _lib.ERR_INVALID_ARG
    assert fwd(m=1) == _lib.ERR_INVALID_ARG              # 40 samples complete no frame of 64
    assert fwd(C=65536) == _lib.ERR_UNSUPPORTED
    X = torch.zeros(2, 1, 33, dtype=torch.complex128, **dev)
    tail = torch.zeros(2, 48, dtype=torch.float64, **dev)
    y = torch.zeros(2, 16, dtype=torch.float64, **dev)

    def inv_call(X=P(X), rows=2, m=1, window=P(w), tail=P(tail), skip=0, o=P(y), n_out=16, wl=64):
        return lib.pbbss_istft_stream(h, X, 1, rows, m, 33, 33, 1, 64, 16, wl, window, tail, skip,
                                      o, n_out, None)
    assert inv_call() == _lib.OK
    assert inv_call(X=None) == _lib.ERR_INVALID_ARG and inv_call(tail=None) == _lib.ERR_INVALID_ARG
    assert inv_call(window=None) == _lib.ERR_INVALID_ARG and inv_call(o=None) == _lib.ERR_INVALID_ARG
    assert inv_call(m=0) == _lib.ERR_INVALID_ARG and inv_call(m=-1) == _lib.ERR_INVALID_ARG
    assert inv_call(n_out=15) == _lib.ERR_INVALID_ARG and inv_call(skip=49) == _lib.ERR_INVALID_ARG
    assert inv_call(wl=56) == _lib.ERR_INVALID_ARG       # no multiple of shift
    assert inv_call(rows=65536) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()


def _stream_results():
    """A forward and an inverse stream, every result of every call."""
    import torch
    from pb_bss_amd.transform import OnlineISTFT, OnlineSTFT
    size, shift, wl, n = so.CASES[4]
    x = torch.from_numpy(_samples(3, n, seed=21)).cuda()
    fwd = OnlineSTFT(3, size, shift, window_length=wl)
    out = [fwd.step_block(b) for b in so.split(x, so.blockings(n, shift, wl, size)['irregular'])]
    out.append(fwd.flush())
    X = torch.from_numpy(_spectra((3,), so.FRAMES, size // 2 + 1, seed=22)).cuda()
    inv = OnlineISTFT(size, shift, window_length=wl, fading=False)
    out += [inv.step_block(b) for b in
            so.split(X, so.frame_blockings(so.FRAMES, wl // shift, size)['irregular'], -2)]
    out.append(inv.flush())
    return [o.cpu() for o in out]


def test_streams_do_not_depend_on_what_the_handle_ran_before():
    """The stream entry points take no memory of the handle (tests/test_stream_symbols.py): behind
    a fit (slabs, control words), an offline istft (work slab) and a WPE they give the bits of a
    fresh handle, and each of those repeats its own first result behind them."""
    import torch
    from oracle import synth
    from pb_bss_amd.distribution import CACGMMTrainer
    from pb_bss_amd.transform import istft, wpe
    from test_gpu_call_order import fresh_handle
    Y, init = synth.make_stft(9, 96, 4, 3, seed=0)
    Yw = np.ascontiguousarray(Y.transpose(0, 2, 1)[:5])                      # (F, D, T)
    X = _spectra((3,), 37, 129, seed=23)

    def fit():
        return CACGMMTrainer().fit(Y, initialization=init, iterations=3).predict(Y)

    predecessors = {'fit': fit, 'istft': lambda: istft(X, 256, 64),
                    'wpe': lambda: wpe(Yw, taps=3, delay=1, iterations=2)}
    with fresh_handle():
        first = _stream_results()
    for name, run in predecessors.items():
        with fresh_handle():
            before = run()
            got = _stream_results()
            after = run()
        assert len(got) == len(first)
        assert all(torch.equal(a, b) for a, b in zip(got, first)), name
        np.testing.assert_array_equal(before, after, err_msg=name)
