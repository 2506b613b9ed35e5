"""kmws_reframe_utf8_workspace_size / kmws_reframe_utf8_batch /
kmws_unpack_reframe_utf8 checks that need no GPU: the symbols exist and are
bound; the workspace holds the reframe's and the validator's per-frame and
per-stream arrays, without its tile plan, on both sides of the copy form's
threshold; every argument check runs before any device work and in the
documented order (the reframe's own values, the stream checks, the workspace
size, the device); without a gfx950 device the entries return
KMWS_ERR_NOT_SUPPORTED (never a CPU fallback)."""
import ctypes as C

import pytest

from kuma_amd import kmws

N, CAP = 5, 1 << 16
UNIT_FROM = 16384  # dst_cap / n from which the copy runs its unit form
S = kmws.SERVER


def test_symbols_exist_and_are_bound():
    L = kmws.lib()
    for name in ("kmws_reframe_utf8_workspace_size", "kmws_reframe_utf8_batch", "kmws_unpack_reframe_utf8"):
        assert hasattr(L, name), name
        assert name in kmws.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert callable(kmws.reframe_utf8) and callable(kmws.unpack_reframe_utf8)
    assert kmws.reframe_utf8_workspace_size(N, CAP) == L.kmws_reframe_utf8_workspace_size(N, CAP, 1)
    assert kmws.reframe_utf8_workspace_size(N, CAP, 7) == L.kmws_reframe_utf8_workspace_size(N, CAP, 7)


def test_workspace_size_holds_the_reframes_and_the_frame_arrays():
    L = kmws.lib()
    size, reframe = L.kmws_reframe_utf8_workspace_size, L.kmws_reframe_workspace_size
    # the validator's arrays alone: its workspace less the tile plan in front of them
    arrays = lambda n, k: L.kmws_utf8_workspace_size(0, n, k) - L.kmws_unmask_workspace_size(0)  # noqa: E731
    for n in (0, 1, 255, 256, 257, 2047, 2048, 2049, (1 << 31) - 1):
        per = (0, 1, 16, 300, 4104, UNIT_FROM - 1, UNIT_FROM, UNIT_FROM + 1, 65550)  # both sides of the form threshold
        for cap in sorted({p * max(n, 1) for p in per} | {max(n, 1) * UNIT_FROM - 1, 1 << 36}):
            for k in (0, 1, 2, 37, 1 << 16):
                assert size(n, cap, k) >= reframe(n, cap) + 12 * n + 8 * k, (n, cap, k)
                assert size(n, cap, k) >= reframe(n, cap) + arrays(n, k) - 16, (n, cap, k)
                assert size(n, cap, k) <= reframe(n, cap) + arrays(n, k) + 512, (n, cap, k)  # up to alignment
    for n in (1000, 4097):
        assert size(n, n * UNIT_FROM, 1) > size(n, n * UNIT_FROM - 1, 1)  # the unit form's records, as the copy's
    # the validator's tile plan is not carried
    for n, cap in ((1 << 20, 1 << 32), (65536, 1 << 32)):
        assert size(n, cap, 3) < reframe(n, cap) + L.kmws_utf8_workspace_size(cap, n, 3)


def reframe_call(src, descs, flags, keys, n, dst, off, first, ns, out, ws, ws_bytes, cap=CAP):
    return kmws.lib().kmws_reframe_utf8_batch(src, descs, flags, keys, n, dst, cap, off, first, ns, None, None, out,
                                              ws, ws_bytes, None)


def unpack_call(wire, hdr, n, mode, desc, flags, err, relay, out_mask, keys, dst, off, first, ns, out, ws, ws_bytes,
                cap=CAP):
    return kmws.lib().kmws_unpack_reframe_utf8(wire, 1 << 16, hdr, n, mode, desc, flags, err, relay, out_mask, keys,
                                               dst, cap, off, first, ns, None, None, out, ws, ws_bytes, None)


def test_reframe_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(4096 + 8)
    need = L.kmws_reframe_utf8_workspace_size(N, CAP, 1)
    bad, small = kmws.ERR_INVALID_PARAM, kmws.ERR_BUFFER_TOO_SMALL
    #      src   descs flags keys  n  dst   off   first ns out   ws    bytes
    ok = [fake, fake, fake, fake, N, fake, fake, None, 1, fake, fake, need]
    for i in (0, 1, 2, 5, 6, 9, 10):  # src, descs, flags, dst, wire_off, out_utf8, workspace
        args = list(ok)
        args[i] = None
        assert reframe_call(*args) == bad, i
    for i in (0, 5):  # src, dst: 16-byte aligned
        args = list(ok)
        args[i] = odd
        assert reframe_call(*args) == bad, i
    assert reframe_call(fake, fake, fake, fake, 1 << 31, fake, fake, None, 1, fake, fake, 1 << 62) == bad
    assert reframe_call(fake, fake, fake, fake, N, fake, fake, fake, 1 << 31, fake, fake, 1 << 62) == bad
    # stream_first NULL needs n_streams == 1; no streams cannot hold frames
    assert reframe_call(fake, fake, fake, fake, N, fake, fake, None, 2, fake, fake, need) == bad
    assert reframe_call(fake, fake, fake, fake, N, fake, fake, fake, 0, fake, fake, need) == bad
    # the stream checks stand in front of the workspace size
    assert reframe_call(fake, fake, fake, fake, N, fake, fake, None, 2, fake, fake, 0) == bad
    assert reframe_call(odd, fake, fake, fake, N, fake, fake, None, 1, fake, fake, 0) == bad
    # an empty batch still needs wire_off and the workspace
    need0 = L.kmws_reframe_utf8_workspace_size(0, CAP, 1)
    assert reframe_call(None, None, None, None, 0, None, None, None, 1, None, fake, need0) == bad
    assert reframe_call(None, None, None, None, 0, None, fake, None, 1, None, None, need0) == bad
    for cap in (CAP, UNIT_FROM * N):  # both copy forms
        need = L.kmws_reframe_utf8_workspace_size(N, cap, 1)
        assert reframe_call(*ok[:11], need - 1, cap=cap) == small
        # the reframe's own workspace is not enough: the frame arrays live behind it
        assert reframe_call(*ok[:11], L.kmws_reframe_workspace_size(N, cap), cap=cap) == small
        assert reframe_call(fake, fake, fake, None, N, fake, fake, None, 1, fake, fake, need - 1, cap=cap) == small


def test_unpack_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)
    odd = C.c_void_p(4096 + 8)
    need = L.kmws_reframe_utf8_workspace_size(N, CAP, 1)
    bad, small = kmws.ERR_INVALID_PARAM, kmws.ERR_BUFFER_TOO_SMALL
    #      wire  hdr   n  mode desc  flags err   relay   mask keys  dst   off   first ns out   ws    bytes
    ok = [fake, fake, N, S, fake, fake, fake, 0x0007, 0, fake, fake, fake, None, 1, fake, fake, need]
    # mode, relay_opcodes, out_mask come first: INVALID_PARAM whatever else is wrong
    for i, v in ((3, 7), (3, -1), (7, 0x10000), (7, 0xFFFFFFFF), (8, 2), (8, -1)):
        for ws_bytes in (need, need - 1, 0):
            args = list(ok)
            args[i], args[16] = v, ws_bytes
            assert unpack_call(*args) == bad, (i, v, ws_bytes)
    for i in (0, 1, 4, 5, 10, 11, 14, 15):  # wire, hdr_off, out_desc, out_flags, dst, wire_off, out_utf8, workspace
        args = list(ok)
        args[i] = None
        assert unpack_call(*args) == bad, i
    for i in (0, 10):  # wire, dst: 16-byte aligned
        args = list(ok)
        args[i] = odd
        assert unpack_call(*args) == bad, i
    big = list(ok)
    big[2], big[16] = 1 << 31, 1 << 62
    assert unpack_call(*big) == bad
    for first, ns, ws_bytes in ((fake, 1 << 31, 1 << 62), (None, 2, need), (fake, 0, need), (None, 2, 0)):
        args = list(ok)
        args[12], args[13], args[16] = first, ns, ws_bytes
        assert unpack_call(*args) == bad, (ns, ws_bytes)
    for cap in (CAP, UNIT_FROM * N):
        need = L.kmws_reframe_utf8_workspace_size(N, cap, 1)
        assert unpack_call(*ok[:16], need - 1, cap=cap) == small
        assert unpack_call(*ok[:16], L.kmws_reframe_workspace_size(N, cap), cap=cap) == small
    need0 = L.kmws_reframe_utf8_workspace_size(0, CAP, 1)
    assert unpack_call(None, None, 0, S, None, None, None, 0xFFFF, 1, None, None, None, None, 1, None, fake,
                       need0) == bad


def test_without_device_is_not_supported():
    L = kmws.lib()
    if L.kmws_device_count() > 0:
        pytest.skip("a device is present")
    fake = C.c_void_p(4096)
    ns = kmws.ERR_NOT_SUPPORTED
    for cap in (CAP, UNIT_FROM * N):
        need = L.kmws_reframe_utf8_workspace_size(N, cap, 1)
        assert reframe_call(fake, fake, fake, fake, N, fake, fake, None, 1, fake, fake, need, cap=cap) == ns
        assert reframe_call(fake, fake, fake, None, N, fake, fake, None, 1, fake, fake, need + 64, cap=cap) == ns
        need3 = L.kmws_reframe_utf8_workspace_size(N, cap, 3)
        assert reframe_call(fake, fake, fake, fake, N, fake, fake, fake, 3, fake, fake, need3, cap=cap) == ns
        for mode, relay, out_mask, keys in ((S, 0x0007, 0, fake), (kmws.CLIENT, 0xFFFF, 1, None), (S, 0, 1, None)):
            assert unpack_call(fake, fake, N, mode, fake, fake, None, relay, out_mask, keys, fake, fake, None, 1, fake,
                               fake, need, cap=cap) == ns
    need0 = L.kmws_reframe_utf8_workspace_size(0, CAP, 1)
    assert reframe_call(None, None, None, None, 0, None, fake, None, 1, None, fake, need0) == ns
    assert unpack_call(None, None, 0, S, None, None, None, 0x0007, 0, None, None, fake, None, 1, None, fake,
                       need0) == ns
