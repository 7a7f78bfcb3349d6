"""CPU: the streaming section of the C ABI (include/pbbss_stream.h) against its binding
(`_lib.STREAM_SIGNATURES`) and the built library, by the rules tests/test_capi_symbols.py applies
to include/pbbss.h; and the classification that tests/test_call_order_table.py demands of every
export of `_lib.SIGNATURES`, kept here for the exports of the second table: each is listed with
the reason why it takes no memory of the handle (tests/test_gpu_stft_online.py runs them between
calls that do).  No compute calls."""
import os
import re

from test_capi_symbols import c_parameter_kind, ctypes_parameter_kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'pbbss_stream.h')

# export -> why it is exempt from the call-order rows: the group of NO_HANDLE_MEMORY
# ("frame-recursive kernels: their state lives in tensors of the caller") that it would join
NO_HANDLE_MEMORY = {
    'pbbss_stft_stream':
        'sample history in two caller tensors, counters on the host; LDS only, no workspace',
    'pbbss_istft_stream':
        'overlap tail in a caller tensor, updated in place by its own workgroup; the windowed '
        'frames stay in LDS, no scratch slab as pbbss_istft takes',
}


def header_prototypes():
    with open(HEADER) as f:
        txt = f.read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'//[^\n]*', '', txt)
    protos = {}
    for name, params in re.findall(r'\b(pbbss_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', txt):
        assert name not in protos, name
        params = ' '.join(params.split())
        protos[name] = [] if params in ('', 'void') else [p.strip() for p in params.split(',')]
    assert sorted(protos) == sorted(set(re.findall(r'\b(pbbss_[a-z0-9_]+)\s*\(', txt)))
    return protos


def test_stream_signatures_match_header_prototypes():
    from pb_bss_amd import _lib
    protos = header_prototypes()
    assert len(protos) == 2, sorted(protos)
    assert sorted(_lib.STREAM_SIGNATURES) == sorted(protos)
    mismatches = []
    for name, params in protos.items():
        want = [c_parameter_kind(p) for p in params]
        have = [ctypes_parameter_kind(t) for t in _lib.STREAM_SIGNATURES[name]]
        if want != have:
            mismatches.append((name, want, have))
    assert not mismatches, mismatches
    # handle first, stream last: what _lib.launch assumes
    for name, params in protos.items():
        assert re.search(r'\bpbbss_handle_t\b', params[0]) and params[-1] == 'void* stream', name


def test_library_exports_the_stream_entry_points():
    from pb_bss_amd import _lib
    lib = _lib.load()
    for name in _lib.STREAM_SIGNATURES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.STREAM_SIGNATURES[name], name
        assert name in _lib._CONVERTERS, name   # reachable through _lib.launch
    import pytest
    with pytest.raises(KeyError):
        _lib.launch_stream('wpe', None)             # only the names of the second table


def test_the_two_tables_are_disjoint_and_the_first_is_untouched():
    from pb_bss_amd import _lib
    assert not set(_lib.STREAM_SIGNATURES) & set(_lib.SIGNATURES)
    assert _lib.EXPORTS == tuple(_lib.SIGNATURES)
    assert not set(_lib.STREAM_SIGNATURES) & set(_lib.EXPORTS)
    assert _lib.load().pbbss_version() == 610
    with open(os.path.join(ROOT, 'include', 'pbbss.h')) as f:
        assert 'pbbss_stft_stream' not in f.read()


def test_every_stream_entry_is_classified():
    from pb_bss_amd import _lib
    assert set(NO_HANDLE_MEMORY) == set(_lib.STREAM_SIGNATURES)
    assert all(len(reason.split()) >= 3 for reason in NO_HANDLE_MEMORY.values())
    # the claim, as far as source text can show it: the boundary of the stream entry points never
    # touches the handle's slabs, control words or team buffer
    with open(os.path.join(ROOT, 'pb_bss_amd', 'csrc', 'capi_stft_stream.hip')) as f:
        text = re.sub(r'//[^\n]*', '', f.read())
    for member in ('work', 'scratch', 'xbuf', 'grow', 'carve', 'team'):
        assert not re.search(r'\b' + member + r'\b', text), member
