"""kmws_reframe_workspace_size / kmws_reframe_batch / kmws_unpack_reframe checks
that need no GPU: the symbols exist, the workspace holds the copy's, every
argument check runs before any device work and in the documented order
(kmws_encode_batch's / kmws_unpack_gather's, on the reframe's workspace size),
without a gfx950 device the entries return KMWS_ERR_NOT_SUPPORTED (never a CPU
fallback), and KMWS_FLAG_SKIP collides with no bit the other entries read."""
import ctypes as C
import os
import re

import pytest

from kuma_amd import kmws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, CAP = 5, 1 << 16
UNIT_FROM = 16384  # dst_cap / n from which the copy runs its unit form
S = kmws.SERVER


def test_symbols_exist_and_are_bound():
    L = kmws.lib()
    for name in ("kmws_reframe_workspace_size", "kmws_reframe_batch", "kmws_unpack_reframe"):
        assert hasattr(L, name), name
        assert name in kmws.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert callable(kmws.reframe_batch) and callable(kmws.unpack_reframe)
    assert kmws.reframe_workspace_size(N, CAP) == L.kmws_reframe_workspace_size(N, CAP)


def test_flag_skip_collides_with_nothing():
    txt = open(os.path.join(ROOT, "include", "kmws_gpu.h")).read()
    skip = int(re.search(r"#define\s+KMWS_FLAG_SKIP\s+(0x[0-9A-Fa-f]+)u", txt).group(1), 16)
    mask = int(re.search(r"#define\s+KMWS_FLAG_MASK\s+(0x[0-9A-Fa-f]+)u", txt).group(1), 16)
    assert skip == kmws.FLAG_SKIP == 0x8000 and mask == kmws.FLAG_MASK
    assert skip & 0xFF == 0 and skip & mask == 0 and skip & 0x1FF == 0
    assert skip < 1 << 16 and bin(skip).count("1") == 1  # one bit of the 16-bit flags word


def test_workspace_size_holds_the_copys():
    L = kmws.lib()
    size, copy = L.kmws_reframe_workspace_size, L.kmws_copy_workspace_size
    ns = (0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 65536, 1 << 20, (1 << 31) - 1)
    for n in ns:
        per = (0, 1, 16, 300, 4104, UNIT_FROM - 1, UNIT_FROM, UNIT_FROM + 1, 65550)  # both sides of the form threshold
        for cap in sorted({p * max(n, 1) for p in per} | {max(n, 1) * UNIT_FROM - 1, 1 << 36}):
            assert size(n, cap) >= copy(n, cap) + 2 * n, (n, cap)
            assert size(n, cap) <= copy(n, cap) + 2 * n + 512, (n, cap)  # the outgoing flags, up to alignment
    for n in (1000, 4097):
        assert (n * (UNIT_FROM - 1)) // n < UNIT_FROM <= (n * UNIT_FROM) // n
        assert size(n, n * UNIT_FROM) > size(n, n * UNIT_FROM - 1)  # the unit form's records, as the copy's


def reframe_call(src, descs, flags, keys, n, dst, off, ws, ws_bytes, cap=CAP):
    return kmws.lib().kmws_reframe_batch(src, descs, flags, keys, n, dst, cap, off, ws, ws_bytes, None)


def unpack_call(wire, hdr, n, mode, desc, flags, err, relay, out_mask, keys, dst, off, ws, ws_bytes, cap=CAP):
    return kmws.lib().kmws_unpack_reframe(wire, 1 << 16, hdr, n, mode, desc, flags, err, relay, out_mask, keys, dst,
                                          cap, off, ws, ws_bytes, None)


def test_reframe_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(4096 + 8)
    need = L.kmws_reframe_workspace_size(N, CAP)
    bad, small = kmws.ERR_INVALID_PARAM, kmws.ERR_BUFFER_TOO_SMALL
    ok = [fake, fake, fake, fake, N, fake, fake, fake, need]
    for i in (0, 1, 2, 5, 6, 7):  # src, descs, flags, dst, wire_off, workspace
        args = list(ok)
        args[i] = None
        assert reframe_call(*args) == bad, i
    for i in (0, 5):  # src, dst: 16-byte aligned
        args = list(ok)
        args[i] = odd
        assert reframe_call(*args) == bad, i
    # an empty batch still needs wire_off and the workspace
    need0 = L.kmws_reframe_workspace_size(0, CAP)
    assert reframe_call(None, None, None, None, 0, None, None, fake, need0) == bad
    assert reframe_call(None, None, None, None, 0, None, fake, None, need0) == bad
    for cap in (CAP, UNIT_FROM * N):  # both copy forms
        need = L.kmws_reframe_workspace_size(N, cap)
        assert reframe_call(*ok[:8], need - 1, cap=cap) == small
        assert reframe_call(*ok[:8], 0, cap=cap) == small
    # kmws_encode_batch's order: with a workspace that is too small, that is what any failing call reports
    assert reframe_call(None, fake, fake, fake, N, fake, fake, fake, need - 1, cap=UNIT_FROM * N) == small
    assert L.kmws_encode_batch(None, fake, fake, N, fake, UNIT_FROM * N, fake, fake, 1, None) == small
    assert L.kmws_encode_batch(None, fake, fake, N, fake, CAP, fake, fake, 1 << 30, None) == bad


def test_unpack_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)
    odd = C.c_void_p(4096 + 8)
    need = L.kmws_reframe_workspace_size(N, CAP)
    bad, small = kmws.ERR_INVALID_PARAM, kmws.ERR_BUFFER_TOO_SMALL
    #      wire  hdr   n  mode desc  flags err   relay   mask keys  dst   off   ws    bytes
    ok = [fake, fake, N, S, fake, fake, fake, 0x0007, 0, fake, fake, fake, fake, need]
    # mode, relay_opcodes, out_mask come first: INVALID_PARAM even with a workspace that is too small
    for i, v in ((3, 7), (3, -1), (7, 0x10000), (7, 0xFFFFFFFF), (8, 2), (8, -1)):
        for ws_bytes in (need, need - 1, 0):
            args = list(ok)
            args[i], args[13] = v, ws_bytes
            assert unpack_call(*args) == bad, (i, v, ws_bytes)
    for i in (0, 1, 4, 10, 11, 12):  # wire, hdr_off, out_desc, dst, wire_off, workspace
        args = list(ok)
        args[i] = None
        assert unpack_call(*args) == bad, i
    for i in (0, 10):  # wire, dst: 16-byte aligned
        args = list(ok)
        args[i] = odd
        assert unpack_call(*args) == bad, i
    for cap in (CAP, UNIT_FROM * N):
        need = L.kmws_reframe_workspace_size(N, cap)
        assert unpack_call(*ok[:13], need - 1, cap=cap) == small
        # the copy's own workspace is not enough: the outgoing flags live behind it
        assert unpack_call(*ok[:13], L.kmws_copy_workspace_size(N, cap), cap=cap) == small
    need0 = L.kmws_reframe_workspace_size(0, CAP)
    assert unpack_call(None, None, 0, S, None, None, None, 0xFFFF, 1, None, None, None, fake, need0) == bad


def test_without_device_is_not_supported():
    L = kmws.lib()
    if L.kmws_device_count() > 0:
        pytest.skip("a device is present")
    fake = C.c_void_p(4096)
    ns = kmws.ERR_NOT_SUPPORTED
    for cap in (CAP, UNIT_FROM * N):
        need = L.kmws_reframe_workspace_size(N, cap)
        assert reframe_call(fake, fake, fake, fake, N, fake, fake, fake, need, cap=cap) == ns
        assert reframe_call(fake, fake, fake, None, N, fake, fake, fake, need + 64, cap=cap) == ns  # out_keys NULL
        for mode, relay, out_mask, keys in ((S, 0x0007, 0, fake), (kmws.CLIENT, 0xFFFF, 1, None), (S, 0, 1, None)):
            assert unpack_call(fake, fake, N, mode, fake, None, None, relay, out_mask, keys, fake, fake, fake, need,
                               cap=cap) == ns
    need0 = L.kmws_reframe_workspace_size(0, CAP)
    assert reframe_call(None, None, None, None, 0, None, fake, fake, need0) == ns
    assert unpack_call(None, None, 0, S, None, None, None, 0x0007, 0, None, None, fake, fake, need0) == ns
