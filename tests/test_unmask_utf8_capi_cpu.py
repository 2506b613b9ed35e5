"""kmws_unmask_utf8_workspace_size / kmws_unmask_utf8_batch /
kmws_unpack_unmask_utf8 checks that need no GPU: the workspace size is monotone
in each argument and holds kmws_utf8_validate's; every argument check runs
before any device work, with kmws_utf8_validate's codes; without a gfx950
device the entries return KMWS_ERR_NOT_SUPPORTED (never a CPU fallback)."""
import ctypes as C

import pytest

from kuma_amd import kmws

SPAN, N = 1 << 16, 5


def test_workspace_size_is_monotone_and_holds_the_validators():
    L = kmws.lib()
    spans = [0, 1, 16384, 16385, 1 << 20, (1 << 20) + 1, 1 << 32, 1 << 36]
    ns = [0, 1, 255, 256, 257, 65536, 1 << 20, (1 << 31) - 1]
    streams = [0, 1, 2, 37, 1 << 16, 1 << 24]
    size = L.kmws_unmask_utf8_workspace_size
    for sp in spans:
        for n in ns:
            for k in streams:
                assert size(sp, n, k) >= L.kmws_utf8_workspace_size(sp, n, k) >= L.kmws_unmask_workspace_size(sp)
    for n in ns:
        for k in streams:
            v = [size(sp, n, k) for sp in spans]
            assert v == sorted(v) and v[0] < v[-1]
    for sp in spans:
        for k in streams:
            v = [size(sp, n, k) for n in ns]
            assert v == sorted(v) and v[0] < v[-1]
        for n in ns:
            v = [size(sp, n, k) for k in streams]
            assert v == sorted(v) and v[0] < v[-1]
    # the saved look-back: at least 4 B per 16 KiB tile on top of the validator's workspace
    assert size(1 << 30, 100, 1) >= L.kmws_utf8_workspace_size(1 << 30, 100, 1) + 4 * (1 << 16)
    assert kmws.unmask_utf8_workspace_size(1 << 20, 100) == size(1 << 20, 100, 1)


def batch_call(base, descs, flags, n, first, ns, out, ws, ws_bytes, sched=-1):
    return kmws.lib().kmws_unmask_utf8_batch(base, SPAN, descs, flags, n, first, ns, None, None, out, ws, ws_bytes,
                                             sched, None)


def unpack_call(wire, hdr, n, mode, desc, flags, first, ns, out, ws, ws_bytes, sched=-1):
    return kmws.lib().kmws_unpack_unmask_utf8(wire, SPAN, hdr, n, mode, desc, flags, None, first, ns, None, None, out,
                                              ws, ws_bytes, sched, None)


def test_batch_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(4096 + 8)
    need = L.kmws_unmask_utf8_workspace_size(SPAN, N, 1)
    bad = kmws.ERR_INVALID_PARAM
    assert batch_call(None, fake, fake, N, None, 1, fake, fake, need) == bad
    assert batch_call(fake, None, fake, N, None, 1, fake, fake, need) == bad
    assert batch_call(fake, fake, None, N, None, 1, fake, fake, need) == bad
    assert batch_call(fake, fake, fake, N, None, 1, None, fake, need) == bad
    assert batch_call(fake, fake, fake, N, None, 1, fake, None, need) == bad
    assert batch_call(odd, fake, fake, N, None, 1, fake, fake, need) == bad
    assert batch_call(fake, fake, fake, 1 << 31, None, 1, fake, fake, 1 << 40) == bad
    assert batch_call(fake, fake, fake, N, fake, 1 << 31, fake, fake, 1 << 40) == bad
    # stream_first NULL needs n_streams == 1; no streams cannot hold frames
    assert batch_call(fake, fake, fake, N, None, 2, fake, fake, need) == bad
    assert batch_call(fake, fake, fake, N, fake, 0, fake, fake, need) == bad
    # schedule codes: an unknown kind, both store policies at once, a stray bit
    for sched in (6, 200, kmws.SCHED_SPLIT4 | kmws.SCHED_NT_STORES | kmws.SCHED_TEMPORAL_STORES, 1 << 20):
        assert batch_call(fake, fake, fake, N, None, 1, fake, fake, need, sched) == bad, sched
    assert batch_call(fake, fake, fake, N, None, 1, fake, fake, need - 1) == kmws.ERR_BUFFER_TOO_SMALL
    assert batch_call(fake, fake, fake, N, None, 1, fake, fake, L.kmws_utf8_workspace_size(SPAN, N, 1)) == \
        kmws.ERR_BUFFER_TOO_SMALL


def test_unpack_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)
    odd = C.c_void_p(4096 + 8)
    need = L.kmws_unmask_utf8_workspace_size(SPAN, N, 1)
    bad = kmws.ERR_INVALID_PARAM
    S = kmws.SERVER
    assert unpack_call(None, fake, N, S, fake, fake, None, 1, fake, fake, need) == bad
    assert unpack_call(fake, None, N, S, fake, fake, None, 1, fake, fake, need) == bad
    assert unpack_call(fake, fake, N, S, None, fake, None, 1, fake, fake, need) == bad
    assert unpack_call(fake, fake, N, S, fake, None, None, 1, fake, fake, need) == bad  # the verdicts need the flags
    assert unpack_call(fake, fake, N, S, fake, fake, None, 1, None, fake, need) == bad
    assert unpack_call(fake, fake, N, S, fake, fake, None, 1, fake, None, need) == bad
    assert unpack_call(odd, fake, N, S, fake, fake, None, 1, fake, fake, need) == bad
    assert unpack_call(fake, fake, N, 7, fake, fake, None, 1, fake, fake, need) == bad
    assert unpack_call(fake, fake, 1 << 31, S, fake, fake, None, 1, fake, fake, 1 << 40) == bad
    assert unpack_call(fake, fake, N, S, fake, fake, fake, 1 << 31, fake, fake, 1 << 40) == bad
    assert unpack_call(fake, fake, N, S, fake, fake, None, 2, fake, fake, need) == bad
    assert unpack_call(fake, fake, N, S, fake, fake, fake, 0, fake, fake, need) == bad
    assert unpack_call(fake, fake, N, S, fake, fake, None, 1, fake, fake, need, 6) == bad
    assert unpack_call(fake, fake, N, S, fake, fake, None, 1, fake, fake, need - 1) == kmws.ERR_BUFFER_TOO_SMALL


def test_without_device_is_not_supported():
    L = kmws.lib()
    if L.kmws_device_count() > 0:
        pytest.skip("a device is present")
    fake = C.c_void_p(4096)
    need = L.kmws_unmask_utf8_workspace_size(SPAN, N, 1)
    assert batch_call(fake, fake, fake, N, None, 1, fake, fake, need) == kmws.ERR_NOT_SUPPORTED
    assert batch_call(fake, fake, fake, N, None, 1, fake, fake, need, kmws.SCHED_SPLIT8 | kmws.SCHED_TEMPORAL_STORES) == \
        kmws.ERR_NOT_SUPPORTED
    assert batch_call(None, None, None, 0, None, 1, None, None, 0) == kmws.ERR_NOT_SUPPORTED
    assert unpack_call(fake, fake, N, kmws.SERVER, fake, fake, None, 1, fake, fake, need) == kmws.ERR_NOT_SUPPORTED
    assert unpack_call(None, None, 0, kmws.SERVER, None, None, None, 1, None, None, 0) == kmws.ERR_NOT_SUPPORTED
