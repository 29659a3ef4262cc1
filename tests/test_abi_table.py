"""cliora_amd._lib: the ABI table against include/cliora_chart.h and the built library, the one refusal of an absent symbol, and the
pointer / device helpers on their CPU cases."""
import ctypes as C
import os
import re

import pytest
import torch

from cliora_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'cliora_chart.h')


def header_prototypes():
    """name -> number of parameters of every cliora_* function the header declares."""
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    protos = {}
    for name, params in re.findall(r'\b(cliora_\w+)\s*\(([^()]*)\)\s*;', text):
        params = params.strip()
        protos[name] = 0 if params in ('', 'void') else params.count(',') + 1
    return protos


def test_table_agrees_with_the_header_and_the_library():
    protos = header_prototypes()
    assert len(protos) > 50, sorted(protos)             # the parse found the header's prototypes, not a handful
    assert sorted(_lib.ABI) == sorted(protos)
    for name, (_, argtypes) in _lib.ABI.items():
        assert len(argtypes) == protos[name], name
    lib = _lib.lib()
    for name, (restype, argtypes) in _lib.ABI.items():
        f = _lib.fn(name)                               # resolves in the freshly built library ...
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name      # ... with the table's types applied
        assert getattr(lib, name) is f


def test_absent_symbol_is_one_refusal():
    class Stub(object):                                 # a library object that lacks cliora_knn_ip, as an older build would
        cliora_version = staticmethod(lambda: b'stub')

    assert _lib.fn('cliora_version', Stub())() == b'stub'
    with pytest.raises(_lib.ChartLibError) as e:
        _lib.fn('cliora_knn_ip', Stub())
    assert str(e.value) == '%s has no cliora_knn_ip: rebuild it (python -m cliora_amd.build)' % _lib.LIB_PATH
    assert _lib.fn('cliora_knn_ip') is _lib.lib().cliora_knn_ip       # the stand-in left nothing behind in the cache of bound functions


def test_pointer_and_device_helpers_on_the_cpu():
    for p in (_lib.ptr(None), _lib.ptr_or_null(None), _lib.ptr_or_null(torch.zeros(4)[:0])):
        assert isinstance(p, C.c_void_p) and not p.value
    t = torch.zeros(3)
    assert _lib.ptr(t).value == t.data_ptr() == _lib.ptr_or_null(t).value
    from cliora_amd import diora
    assert diora._ptr is _lib.ptr and diora._stream is _lib.stream and diora._param_struct is _lib.param_struct
    st = _lib.param_struct({'leaf_w': t})
    assert st.leaf_w == t.data_ptr() and st.leaf_b is None
    for x in (None, t):                                 # nothing to enter: no CUDA call is made for either
        g = _lib.device_guard(x)
        assert g.ctx is None
        with g:
            pass
