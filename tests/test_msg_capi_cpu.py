"""The message index without a GPU: the symbols and their bindings, kmws_msg's
48 bytes in the header, the ctypes structure and the numpy dtype, the workspace
size, and kmws_msg_index's argument checks (before any device work, in the
documented order; KMWS_ERR_NOT_SUPPORTED without a device, never a CPU
fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from kuma_amd import kmws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_bound():
    L = kmws.lib()
    for name in ("kmws_msg_workspace_size", "kmws_msg_index"):
        assert name in kmws.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert L.kmws_msg_index.restype is C.c_int and len(L.kmws_msg_index.argtypes) == 18
    assert L.kmws_msg_workspace_size.restype is C.c_size_t
    assert (kmws.MSG_NONE, kmws.MSG_BEGIN, kmws.MSG_END, kmws.MSG_CONTIG) == (0xFFFFFFFF, 1, 2, 4)
    hdr = open(os.path.join(ROOT, "include", "kmws_gpu.h")).read()
    for name, value in (("NONE", "0xFFFFFFFFu"), ("BEGIN", "1u"), ("END", "2u"), ("CONTIG", "4u")):
        assert re.search(rf"#define KMWS_MSG_{name}\s+{value}\b", hdr), name


def test_record_is_48_bytes_in_every_view():
    offsets = dict(off=0, bytes=8, prior=16, stream=24, first=28, last=32, frames=36, b0=40, bits=41, utf8=42,
                   proto=43, reserved=44)
    assert C.sizeof(kmws.Msg) == 48
    assert {name: getattr(kmws.Msg, name).offset for name, _ in kmws.Msg._fields_} == offsets
    dt = kmws.msg_dtype()
    assert dt.itemsize == 48 and {name: dt.fields[name][1] for name in dt.names} == offsets
    assert [name for name, _ in kmws.Msg._fields_] == list(dt.names)
    for name, ctype in kmws.Msg._fields_:
        assert C.sizeof(ctype) == dt.fields[name][0].itemsize, name
    # the same record through both
    m = kmws.Msg(off=1 << 40, bytes=(1 << 33) + 1, prior=7, stream=3, first=4, last=9, frames=5, b0=0x42, bits=5,
                 utf8=2, proto=10)
    a = np.frombuffer(bytes(m), dtype=dt)[0]
    assert [int(a[name]) for name in dt.names] == [1 << 40, (1 << 33) + 1, 7, 3, 4, 9, 5, 0x42, 5, 2, 10, 0]


def test_workspace_size_is_monotone_and_small():
    size = kmws.lib().kmws_msg_workspace_size
    ns = [0, 1, 1023, 1024, 1025, 65536, 1 << 20, (1 << 23) + 1, (1 << 31) - 1]
    streams = [0, 1, 2, 1023, 1024, 1 << 16, 1 << 24, (1 << 31) - 1]
    for k in streams:
        v = [size(n, k) for n in ns]
        assert v == sorted(v) and v[0] < v[-1]
    for n in ns:
        v = [size(n, k) for k in streams]
        assert v == sorted(v)  # it grows only where the streams need more blocks than the frames
        assert n >= 1 << 23 or v[0] < v[-1]
    # head | 4 + 4 B per block of frames or streams | 24 + 24 B per block of frames and the total | 2 B per frame
    # in whole blocks of 1024; every region rounded up to 16 B
    n, k = 1 << 23, 1 << 16
    blocks = n // 1024
    assert size(n, k) == 16 + 2 * 4 * blocks + 24 * blocks + 24 * (blocks + 1) + 8 + 2 * n
    assert size(n, k) <= 2 * n + 56 * blocks + 64
    assert size(1, 1 << 20) <= 2 * 1024 + 8 * 1025 + 48 * 2 + 80  # the stream blocks hold state aggregates only
    assert kmws.msg_workspace_size(100) == size(100, 1)


def test_index_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    need = L.kmws_msg_workspace_size(5, 1)
    v = L.kmws_msg_index
    inv = kmws.ERR_INVALID_PARAM
    big = 1 << 40
    #          descs flags pos   utf8  proto n  first ns carries     msg_of msgs  cap count smf   ws    bytes stream
    assert v(None, fake, None, None, None, 5, None, 1, None, None, None, fake, 5, fake, None, fake, need, None) == inv
    assert v(fake, None, None, None, None, 5, None, 1, None, None, None, fake, 5, fake, None, fake, need, None) == inv
    assert v(fake, fake, None, None, None, 5, None, 1, None, None, None, None, 5, fake, None, fake, need, None) == inv
    assert v(fake, fake, None, None, None, 5, None, 1, None, None, None, fake, 5, None, None, fake, need, None) == inv
    assert v(fake, fake, None, None, None, 5, None, 1, None, None, None, fake, 5, fake, None, None, need, None) == inv
    assert v(fake, fake, None, None, None, 1 << 31, None, 1, None, None, None, fake, 5, fake, None, fake, big, None) == inv
    assert v(fake, fake, None, None, None, 5, fake, 1 << 31, None, None, None, fake, 5, fake, None, fake, big, None) == inv
    # stream_first NULL needs n_streams == 1; no streams cannot hold frames
    assert v(fake, fake, None, None, None, 5, None, 2, None, None, None, fake, 5, fake, None, fake, need, None) == inv
    assert v(fake, fake, None, None, None, 5, fake, 0, None, None, None, fake, 5, fake, None, fake, need, None) == inv
    # msg_count and workspace are needed without frames too
    assert v(None, None, None, None, None, 0, None, 1, None, None, None, None, 0, None, None, fake, 0, None) == inv
    assert v(None, None, None, None, None, 0, None, 1, None, None, None, None, 0, fake, None, None, 0, None) == inv
    # every INVALID_PARAM comes before BUFFER_TOO_SMALL
    assert v(None, fake, None, None, None, 5, None, 1, None, None, None, fake, 5, fake, None, fake, 0, None) == inv
    assert v(fake, fake, None, None, None, 5, None, 1, None, None, None, None, 5, fake, None, fake, 0, None) == inv
    assert v(fake, fake, None, None, None, 5, None, 2, None, None, None, fake, 5, fake, None, fake, 0, None) == inv
    assert v(fake, fake, None, None, None, 1 << 31, None, 1, None, None, None, fake, 5, fake, None, fake, 0, None) == inv
    small = kmws.ERR_BUFFER_TOO_SMALL
    assert v(fake, fake, None, None, None, 5, None, 1, None, None, None, fake, 5, fake, None, fake, need - 1, None) == small
    assert v(fake, fake, fake, fake, fake, 5, None, 1, fake, fake, fake, fake, 0, fake, fake, fake, 0, None) == small


def test_index_without_device_is_not_supported():
    L = kmws.lib()
    if L.kmws_device_count() > 0:
        pytest.skip("a device is present")
    fake = C.c_void_p(4096)
    need = L.kmws_msg_workspace_size(5, 1)
    assert L.kmws_msg_index(fake, fake, None, None, None, 5, None, 1, None, None, None, fake, 5, fake, None, fake, need,
                            None) == kmws.ERR_NOT_SUPPORTED
    assert L.kmws_msg_index(None, None, None, None, None, 0, None, 1, None, None, None, None, 0, fake, None, fake, 0,
                            None) == kmws.ERR_NOT_SUPPORTED
