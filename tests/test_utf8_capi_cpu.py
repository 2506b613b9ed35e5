"""kmws_utf8_workspace_size / kmws_utf8_validate checks that need no GPU: the
workspace size is monotone in each argument and holds the unmask plan; the
argument checks run before any device work; without a gfx950 device the entry
returns KMWS_ERR_NOT_SUPPORTED (never a CPU fallback)."""
import ctypes as C

import pytest

from kuma_amd import kmws


def test_workspace_size_is_monotone_and_holds_the_unmask_plan():
    L = kmws.lib()
    spans = [0, 1, 16384, 16385, 1 << 20, (1 << 20) + 1, 1 << 32, 1 << 36]
    ns = [0, 1, 255, 256, 257, 65536, 1 << 20, (1 << 31) - 1]
    streams = [0, 1, 2, 37, 1 << 16, 1 << 24]
    size = L.kmws_utf8_workspace_size
    for sp in spans:
        for n in ns:
            for k in streams:
                assert size(sp, n, k) >= L.kmws_unmask_workspace_size(sp)
    for n in ns:
        for k in streams:
            v = [size(sp, n, k) for sp in spans]
            assert v == sorted(v)
    for sp in spans:
        for k in streams:
            v = [size(sp, n, k) for n in ns]
            assert v == sorted(v) and v[0] < v[-1]
        for n in ns:
            v = [size(sp, n, k) for k in streams]
            assert v == sorted(v) and v[0] < v[-1]
    assert kmws.utf8_workspace_size(1 << 20, 100) == size(1 << 20, 100, 1)


def test_validate_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(4096 + 8)
    need = L.kmws_utf8_workspace_size(1 << 16, 5, 1)
    v = L.kmws_utf8_validate
    assert v(fake, 1 << 16, None, fake, 5, 0, None, 1, None, None, fake, fake, need, None) == kmws.ERR_INVALID_PARAM
    assert v(fake, 1 << 16, fake, None, 5, 0, None, 1, None, None, fake, fake, need, None) == kmws.ERR_INVALID_PARAM
    assert v(fake, 1 << 16, fake, fake, 5, 0, None, 1, None, None, None, fake, need, None) == kmws.ERR_INVALID_PARAM
    assert v(fake, 1 << 16, fake, fake, 5, 0, None, 1, None, None, fake, None, need, None) == kmws.ERR_INVALID_PARAM
    assert v(odd, 1 << 16, fake, fake, 5, 0, None, 1, None, None, fake, fake, need, None) == kmws.ERR_INVALID_PARAM
    assert v(fake, 1 << 16, fake, fake, 1 << 31, 0, None, 1, None, None, fake, fake, 1 << 40, None) == \
        kmws.ERR_INVALID_PARAM
    # stream_first NULL needs n_streams == 1; no streams cannot hold frames
    assert v(fake, 1 << 16, fake, fake, 5, 0, None, 2, None, None, fake, fake, need, None) == kmws.ERR_INVALID_PARAM
    assert v(fake, 1 << 16, fake, fake, 5, 0, fake, 0, None, None, fake, fake, need, None) == kmws.ERR_INVALID_PARAM
    assert v(fake, 1 << 16, fake, fake, 5, 0, None, 1, None, None, fake, fake, need - 1, None) == \
        kmws.ERR_BUFFER_TOO_SMALL


def test_validate_without_device_is_not_supported():
    L = kmws.lib()
    if L.kmws_device_count() > 0:
        pytest.skip("a device is present")
    fake = C.c_void_p(4096)
    need = L.kmws_utf8_workspace_size(1 << 16, 5, 1)
    assert L.kmws_utf8_validate(fake, 1 << 16, fake, fake, 5, 0, None, 1, None, None, fake, fake, need, None) == \
        kmws.ERR_NOT_SUPPORTED
    assert L.kmws_utf8_validate(None, 0, None, None, 0, 0, None, 1, None, None, None, None, 0, None) == \
        kmws.ERR_NOT_SUPPORTED
