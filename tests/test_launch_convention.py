"""CPU: the calling convention of include/pbbss.h as `_lib.launch` / `_lib.control` spell it
(marshalling from `_lib.SIGNATURES`, against a stub library) and as the sources of the package
use it (which export goes through which of the two).  Needs neither a GPU nor the built
library."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_capi_symbols import ROOT, header_prototypes

# host functions that are not calls on a thread's handle: the only exports a module may call on
# load() itself
HANDLE_LESS = {'pbbss_version', 'pbbss_error_string', 'pbbss_create', 'pbbss_destroy',
               'pbbss_shard_bounds', 'pbbss_stft_num_frames', 'pbbss_bss_eval_workspace',
               'pbbss_comm_unique_id'}


class FakeTensor:
    def __init__(self, address, contiguous=True, cuda=True):
        self.address, self.contiguous, self.is_cuda = address, contiguous, cuda
        self.device = 'fake:0'

    def is_contiguous(self):
        return self.contiguous

    def stride(self):
        return (1,)

    def data_ptr(self):
        return self.address


class StubLibrary:
    """every export: records its arguments, returns `rc`"""

    def __init__(self):
        self.rc = 0
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('pbbss_'):
            raise AttributeError(name)
        if name == 'pbbss_error_string':
            return lambda rc: b'stub error'

        def export(*args):
            self.calls.append((name, args))
            return self.rc
        return export


class FakeStream:
    """stand-in of a torch stream: records the streams it was made to wait for, and how many
    exports had been called by then"""

    def __init__(self, lib, cuda_stream, device_index=0):
        self.lib, self.cuda_stream, self.device_index = lib, cuda_stream, device_index
        self.waits = []

    def wait_stream(self, other):
        self.waits.append((other, len(self.lib.calls)))

    # torch.Stream compares by stream id and device, and answers False to EVERY comparison with
    # None, `!=` included: an ordering that asks `last != stream` never starts
    def __eq__(self, other):
        return other is not None and (self.cuda_stream, self.device_index) == (
            other.cuda_stream, other.device_index)

    def __ne__(self, other):
        return other is not None and not self == other

    __hash__ = object.__hash__


@pytest.fixture
def stub(monkeypatch):
    from pb_bss_amd import _lib
    lib = StubLibrary()
    lib.handle = ctypes.c_void_p(0x1000)
    lib.stream = ctypes.c_void_p(0x2000)
    lib.devices = []
    lib.current = FakeStream(lib, 0x2000)   # what torch.cuda.current_stream() would give
    lib.capturing = False
    lib.capture_queries = 0

    def is_capturing():
        lib.capture_queries += 1
        return lib.capturing

    def handle(device_index=None):
        lib.devices.append(device_index)
        return lib.handle

    monkeypatch.setattr(_lib, 'load', lambda: lib)
    monkeypatch.setattr(_lib, 'handle', handle)
    monkeypatch.setattr(_lib, 'stream_ptr', lambda device_index=None, stream=None: lib.stream)
    monkeypatch.setattr(_lib, 'current_stream', lambda device_index=None: lib.current)
    monkeypatch.setattr(_lib, 'is_capturing', is_capturing)
    monkeypatch.setattr(_lib, '_last_stream', {})
    return lib


def _quantile_args(_lib, x=None):
    geom = _lib.MaskGeom()
    rank = (ctypes.c_int64 * 2)(3, 4)
    gamma = (ctypes.c_double * 2)(0.25, 0.5)
    negative = (ctypes.c_int * 2)(0, 1)
    raw = ctypes.c_void_p(0xabc0)
    out, status = FakeTensor(0x300), FakeTensor(0x400)
    args = [raw if x is None else x, True, geom, np.int64(2), rank, gamma, negative,
            np.float32(0.5), 1, out, np.bool_(False), status]
    return args, dict(geom=geom, rank=rank, gamma=gamma, negative=negative, raw=raw)


def test_launch_marshalling(stub):
    from pb_bss_amd import _lib
    # pbbss_mask_quantile: a POINTER(struct) slot, three array slots, scalars of every kind
    args, obj = _quantile_args(_lib)
    rc = _lib.launch('pbbss_mask_quantile', 0, *args, what='mask_quantile(test)')
    assert rc == 0
    (name, sent), = stub.calls
    assert name == 'pbbss_mask_quantile' and len(sent) == len(_lib.SIGNATURES[name])
    assert sent[0] is stub.handle and sent[-1] is stub.stream  # handle first, stream last
    assert stub.devices == [0]
    assert sent[1] is obj['raw']                               # a c_void_p by identity
    assert sent[2] == 1 and type(sent[2]) is int               # True -> 1
    assert type(sent[3]).__name__ == 'CArgObject'              # a Structure by reference
    assert sent[4] == 2 and type(sent[4]) is int               # np.int64
    assert sent[5] is obj['rank'] and sent[6] is obj['gamma'] and sent[7] is obj['negative']
    assert sent[8] == 0.5 and type(sent[8]) is float           # np.float32
    assert sent[9] == 1.0 and type(sent[9]) is float           # an int in a double slot
    assert isinstance(sent[10], ctypes.c_void_p) and sent[10].value == 0x300
    assert sent[11] == 0 and type(sent[11]) is int
    assert sent[12].value == 0x400

    # a torch.device-like object gives its index
    stub.calls.clear()
    _lib.launch('pbbss_mask_quantile', type('Device', (), {'index': 3})(), *args)
    assert stub.devices[-1] == 3

    # a tensor must be on the device and contiguous; nothing is called otherwise
    stub.calls.clear()
    for bad in (FakeTensor(0x500, contiguous=False), FakeTensor(0x500, cuda=False)):
        with pytest.raises(AssertionError):
            _lib.launch('pbbss_mask_quantile', 0, *_quantile_args(_lib, bad)[0])
    # one argument too few / too many: TypeError naming the export, before any call
    for wrong in (args[:-1], args + [0]):
        with pytest.raises(TypeError, match=r'pbbss_mask_quantile takes 12 arguments'):
            _lib.launch('pbbss_mask_quantile', 0, *wrong)
    assert stub.calls == []

    # pbbss_cacgmm_fit: many optional pointers (None -> NULL), the options by reference
    y = FakeTensor(0x700)
    opts = _lib.EmOpts(iterations=3)
    outs = [FakeTensor(0x800 + 16 * i) for i in range(4)]
    fit = [y, np.int64(7), 5, 4, 3, None, None, None, None, None, None, opts, *outs, None, None]
    _lib.launch('pbbss_cacgmm_fit', None, *fit)
    (name, sent), = stub.calls
    assert len(sent) == len(_lib.SIGNATURES['pbbss_cacgmm_fit']) and stub.devices[-1] is None
    assert sent[0] is stub.handle and sent[-1] is stub.stream
    assert sent[1].value == 0x700 and sent[2] == 7 and type(sent[2]) is int
    assert sent[6:12] == (None,) * 6 and sent[17:19] == (None, None)
    assert type(sent[12]).__name__ == 'CArgObject'
    assert [p.value for p in sent[13:17]] == [0x800, 0x810, 0x820, 0x830]
    # pbbss_cacgmm_predict: a double slot between integers
    pred = [y, 2, 5, 4, 3, y, y, y, 3, 1, 0, None, 0, True, np.float32(0.5), y, None, None]
    stub.calls.clear()
    _lib.launch('pbbss_cacgmm_predict', 0, *pred)
    sent = stub.calls[0][1]
    assert sent[15] == 0.5 and type(sent[15]) is float and sent[14] == 1 and type(sent[14]) is int

    # return codes
    stub.rc = _lib.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match=r'^cacgmm_fit\(test\): '):
        _lib.launch('pbbss_cacgmm_fit', 0, *fit, what='cacgmm_fit(test)')
    with pytest.raises(NotImplementedError, match=r'^pbbss_cacgmm_fit: '):
        _lib.launch('pbbss_cacgmm_fit', 0, *fit)
    assert _lib.launch('pbbss_cacgmm_fit', 0, *fit, accept=(_lib.ERR_UNSUPPORTED,)) == -2
    stub.rc = _lib.ERR_HIP
    with pytest.raises(_lib.PbbssError, match=r'cacgmm_fit\(test\): .*\(code -3\)'):
        _lib.launch('pbbss_cacgmm_fit', 0, *fit, what='cacgmm_fit(test)',
                    accept=(_lib.ERR_UNSUPPORTED,))
    with pytest.raises(_lib.PbbssError):
        _lib.control('pbbss_split_reset', 0)

    # control: the handle and no stream; a scalar ctypes object goes by reference
    stub.rc = 0
    stub.calls.clear()
    ms = ctypes.c_float()
    assert _lib.control('pbbss_kernel_ms_lagged', 1, np.int64(2), ms, what='kernel_ms_lagged') == 0
    _lib.control('pbbss_set_split_tail', None, True)
    _lib.control('pbbss_comm_create', 0, b'u' * 128, 2, 1)
    _lib.control('pbbss_split_reset', 0)
    lagged, tail, comm, reset = (sent for _, sent in stub.calls)
    assert lagged[0] is stub.handle and lagged[1] == 2 and len(lagged) == 3
    assert type(lagged[2]).__name__ == 'CArgObject'
    assert tail == (stub.handle, 1) and type(tail[1]) is int
    assert comm[1] == b'u' * 128 and reset == (stub.handle,)
    assert stub.devices[-4:] == [1, None, 0, 0]
    with pytest.raises(TypeError, match=r'pbbss_set_split_tail takes 1 argument'):
        _lib.control('pbbss_set_split_tail', 0)

    # view_ptr: any view on the device
    assert _lib.view_ptr(FakeTensor(0x900, contiguous=False)).value == 0x900
    with pytest.raises(AssertionError):
        _lib.view_ptr(FakeTensor(0x900, cuda=False))


def test_launch_orders_a_new_stream_behind_the_previous_one(stub):
    """Consecutive calls on one handle share its workspaces: `launch` remembers, per handle key,
    the stream of the last launch and makes another stream wait for it before the export runs."""
    import threading
    from pb_bss_amd import _lib
    me = threading.get_ident()

    def call(device=0):                         # any export with a stream will do
        _lib.launch('pbbss_heev_batched', device, None, 1, 2, None, None, None)

    a, b, c = stub.current, FakeStream(stub, 0x2100), FakeStream(stub, 0x2200)
    call()                                     # the first launch of the key: nothing to wait for
    assert a.waits == [] and _lib._last_stream == {(0, me): a}
    queries = stub.capture_queries
    call()
    call()                                     # same stream: no wait, no runtime query at all
    assert a.waits == [] and stub.capture_queries == queries and len(stub.calls) == 3
    stub.current = b                            # switch: one wait, before the export is called
    call()
    assert b.waits == [(a, 3)] and a.waits == [] and len(stub.calls) == 4
    assert _lib._last_stream[(0, me)] is b
    call()
    assert b.waits == [(a, 3)]
    stub.current = a                            # switch back: again one wait
    call()
    assert a.waits == [(b, 5)] and b.waits == [(a, 3)]
    call()
    assert a.waits == [(b, 5)]
    # a capture in progress: nothing is ordered, the remembered stream stays
    stub.current, stub.capturing = c, True
    call()
    call()
    assert c.waits == [] and _lib._last_stream[(0, me)] is a and len(stub.calls) == 9
    stub.current, stub.capturing = a, False
    call()                                     # back on the remembered stream: still no wait
    assert a.waits == [(b, 5)]
    # the remembered stream is kept per handle key: another device starts from nothing ...
    other = FakeStream(stub, 0x2300, device_index=1)
    stub.current = other
    call(1)
    assert other.waits == [] and _lib._last_stream == {(0, me): a, (1, me): other}
    # ... another thread too, and neither disturbs the first key
    seen = {}

    def worker():
        stub.current = b
        call()
        seen['key'] = (0, threading.get_ident())
    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert b.waits == [(a, 3)] and _lib._last_stream[(0, me)] is a
    # (a finished thread's ident may be handed out again: only the entry itself is checked)
    assert _lib._last_stream[seen['key']] is b
    stub.current = a
    call()
    assert a.waits == [(b, 5)]
    # a device given as None is keyed by the device of the current stream
    stub.current = b
    _lib.launch('pbbss_heev_batched', None, None, 1, 2, None, None, None)
    assert b.waits[-1][0] is a and _lib._last_stream[(0, me)] is b


def _package_sources():
    pkg = os.path.join(ROOT, 'pb_bss_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in sorted(files):
            if f.endswith('.py'):
                path = os.path.join(dirpath, f)
                with open(path) as fh:
                    yield os.path.relpath(path, pkg), fh.read()


def test_call_sites_follow_the_convention():
    """Which export the sources of the package reach through `launch`, which through `control`
    and which on the loaded library itself, against the prototypes of the header."""
    protos = header_prototypes()

    def has_handle(name):
        return bool(protos[name]) and re.search(r'\bpbbss_handle_t\b', protos[name][0]) is not None

    def has_stream(name):
        return bool(protos[name]) and re.fullmatch(r'void\s*\*\s*stream', protos[name][-1]) is not None

    launched, controlled, quoted, attribute = set(), set(), set(), set()
    for rel, src in _package_sources():
        launched.update(re.findall(r'\blaunch\(\s*[\'"](pbbss_\w+)[\'"]', src))
        controlled.update(re.findall(r'\bcontrol\(\s*[\'"](pbbss_\w+)[\'"]', src))
        if rel != '_lib.py':
            # the name of an export as a string (not the start of a docstring) or as an
            # attribute of the loaded library
            quoted.update(re.findall(r'(?<![\'"])[\'"](pbbss_\w+)[\'"]', src))
            attribute.update(re.findall(r'\.(pbbss_\w+)\s*\(', src))
            # no call with a computed name slips past the two lists
            assert not re.search(r'_lib\.(launch|control)\(\s*(?![\'"]pbbss_)', src), rel
    assert launched and controlled
    assert launched | controlled | attribute <= set(protos)
    for name in launched:
        assert has_handle(name) and has_stream(name), (name, protos[name])
    for name in controlled:
        assert has_handle(name) and not any('stream' in p for p in protos[name]), name
    assert attribute <= HANDLE_LESS, sorted(attribute - HANDLE_LESS)
    assert all(not has_stream(name) for name in HANDLE_LESS)
    # an export named in the code is named in a launch or a control call
    assert quoted == launched | controlled, sorted(quoted ^ (launched | controlled))
    # every export with a handle and a stream is reached through launch; the unpack kernel of the
    # gather alone is driven by its test only
    streamed = {name for name in protos if has_handle(name) and has_stream(name)}
    assert streamed - launched == {'pbbss_allgather_unpack'}, sorted(streamed - launched)
