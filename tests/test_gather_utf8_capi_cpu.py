"""kmws_gather_utf8_workspace_size / kmws_gather_unmask_utf8 /
kmws_unpack_gather_utf8 checks that need no GPU: the workspace size grows with
each argument inside a copy form and holds the copy's workspace without the
validator's tile plan; every argument check runs before any device work; without
a gfx950 device the entries return KMWS_ERR_NOT_SUPPORTED (never a CPU
fallback)."""
import ctypes as C

import pytest

from kuma_amd import kmws

N, CAP = 5, 1 << 16
UNIT_FROM = 16384  # dst_cap / n from which the copy runs its unit form


def test_workspace_size_is_monotone_and_holds_the_copys():
    L = kmws.lib()
    size = L.kmws_gather_utf8_workspace_size
    streams = [0, 1, 2, 37, 1 << 16, 1 << 24]
    # (n, dst_cap) ascending in both, all in one copy form: the copy's own workspace is smaller in
    # the chunk form, so the size is monotone inside a form, not across the threshold
    chunk = [(1, 16), (255, 1 << 16), (256, 1 << 20), (257, 1 << 22), (65536, 1 << 28), (1 << 20, 1 << 32),
             ((1 << 31) - 1, 1 << 36)]
    unit = [(1, UNIT_FROM), (255, 1 << 22), (256, 1 << 23), (257, 1 << 24), (65536, 1 << 32), (1 << 20, 1 << 36)]
    for form, cases in (("chunk", chunk), ("unit", unit)):
        for n, cap in cases:
            assert (cap // n < UNIT_FROM) == (form == "chunk")
            for k in streams:
                assert size(n, cap, k) >= L.kmws_copy_workspace_size(n, cap) + 12 * n + 8 * k
        for k in streams:
            v = [size(n, cap, k) for n, cap in cases]
            assert v == sorted(v) and v[0] < v[-1], form
        for n, cap in cases:
            v = [size(n, cap, k) for k in streams]
            assert v == sorted(v) and v[0] < v[-1]
        # n alone and dst_cap alone, as far as the form holds
        n, cap = cases[3]
        if form == "chunk":
            vn = [size(m, cap, 1) for m in (n, 2 * n, 100 * n)]
            vc = [size(100 * n, c, 1) for c in (cap, 2 * cap, 50 * cap)]
        else:
            vn = [size(m, cap, 1) for m in (n // 4, n // 2, n)]
            vc = [size(n, c, 1) for c in (cap, 2 * cap, 1000 * cap)]
        assert vn == sorted(vn) and vn[0] < vn[-1] and vc == sorted(vc) and vc[0] < vc[-1], form
    # the validator's tile plan is not carried
    for n, cap in ((1 << 20, 1 << 32), (65536, 1 << 32)):
        assert size(n, cap, 3) < L.kmws_copy_workspace_size(n, cap) + L.kmws_utf8_workspace_size(cap, n, 3)
        # ... and nothing else is added: the validator's arrays, up to alignment
        assert L.kmws_utf8_workspace_size(cap, n, 3) - L.kmws_unmask_workspace_size(cap) - 16 <= \
            size(n, cap, 3) - L.kmws_copy_workspace_size(n, cap) <= \
            L.kmws_utf8_workspace_size(cap, n, 3) - L.kmws_unmask_workspace_size(cap) + 256
    assert kmws.gather_utf8_workspace_size(100, 1 << 20) == size(100, 1 << 20, 1)
    assert size(0, 0, 0) >= L.kmws_copy_workspace_size(0, 0)


def gather_call(src, descs, flags, n, dst, off, first, ns, out, ws, ws_bytes, cap=CAP):
    return kmws.lib().kmws_gather_unmask_utf8(src, descs, flags, n, dst, cap, off, first, ns, None, None, out, ws,
                                              ws_bytes, None)


def unpack_call(wire, hdr, n, mode, desc, flags, dst, off, first, ns, out, ws, ws_bytes, cap=CAP):
    return kmws.lib().kmws_unpack_gather_utf8(wire, 1 << 16, hdr, n, mode, desc, flags, None, dst, cap, off, first, ns,
                                              None, None, out, ws, ws_bytes, None)


def test_gather_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(4096 + 8)
    need = L.kmws_gather_utf8_workspace_size(N, CAP, 1)
    bad = kmws.ERR_INVALID_PARAM
    ok = [fake, fake, fake, N, fake, fake, None, 1, fake, fake, need]
    for i in (0, 1, 2, 4, 5, 8, 9):  # src, descs, flags, dst, dst_off, out_utf8, workspace
        args = list(ok)
        args[i] = None
        assert gather_call(*args) == bad, i
    for i in (0, 4):  # src, dst: 16-byte aligned
        args = list(ok)
        args[i] = odd
        assert gather_call(*args) == bad, i
    assert gather_call(fake, fake, fake, 1 << 31, fake, fake, None, 1, fake, fake, 1 << 62) == bad
    assert gather_call(fake, fake, fake, N, fake, fake, fake, 1 << 31, fake, fake, 1 << 62) == bad
    # stream_first NULL needs n_streams == 1; no streams cannot hold frames
    assert gather_call(fake, fake, fake, N, fake, fake, None, 2, fake, fake, need) == bad
    assert gather_call(fake, fake, fake, N, fake, fake, fake, 0, fake, fake, need) == bad
    # an empty batch still needs dst_off and the workspace
    assert gather_call(None, None, None, 0, None, None, None, 1, None, fake, need) == bad
    assert gather_call(None, None, None, 0, None, fake, None, 1, None, None, need) == bad
    for cap in (CAP, UNIT_FROM * N):  # both copy forms
        need = L.kmws_gather_utf8_workspace_size(N, cap, 1)
        assert gather_call(*ok[:10], need - 1, cap=cap) == kmws.ERR_BUFFER_TOO_SMALL
        assert gather_call(*ok[:10], L.kmws_copy_workspace_size(N, cap), cap=cap) == kmws.ERR_BUFFER_TOO_SMALL


def test_unpack_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)
    odd = C.c_void_p(4096 + 8)
    need = L.kmws_gather_utf8_workspace_size(N, CAP, 1)
    bad = kmws.ERR_INVALID_PARAM
    S = kmws.SERVER
    ok = [fake, fake, N, S, fake, fake, fake, fake, None, 1, fake, fake, need]
    for i in (0, 1, 4, 5, 6, 7, 10, 11):  # wire, hdr_off, out_desc, out_flags, dst, dst_off, out_utf8, workspace
        args = list(ok)
        args[i] = None
        assert unpack_call(*args) == bad, i
    for i in (0, 6):  # wire, dst: 16-byte aligned
        args = list(ok)
        args[i] = odd
        assert unpack_call(*args) == bad, i
    assert unpack_call(fake, fake, N, 7, fake, fake, fake, fake, None, 1, fake, fake, need) == bad
    assert unpack_call(fake, fake, 1 << 31, S, fake, fake, fake, fake, None, 1, fake, fake, 1 << 62) == bad
    assert unpack_call(fake, fake, N, S, fake, fake, fake, fake, fake, 1 << 31, fake, fake, 1 << 62) == bad
    assert unpack_call(fake, fake, N, S, fake, fake, fake, fake, None, 2, fake, fake, need) == bad
    assert unpack_call(fake, fake, N, S, fake, fake, fake, fake, fake, 0, fake, fake, need) == bad
    assert unpack_call(*ok[:12], need - 1) == kmws.ERR_BUFFER_TOO_SMALL


def test_without_device_is_not_supported():
    L = kmws.lib()
    if L.kmws_device_count() > 0:
        pytest.skip("a device is present")
    fake = C.c_void_p(4096)
    need = L.kmws_gather_utf8_workspace_size(N, CAP, 1)
    assert gather_call(fake, fake, fake, N, fake, fake, None, 1, fake, fake, need) == kmws.ERR_NOT_SUPPORTED
    assert gather_call(fake, fake, fake, N, fake, fake, fake, 3, fake, fake, need + 64) == kmws.ERR_NOT_SUPPORTED
    need0 = L.kmws_gather_utf8_workspace_size(0, CAP, 1)
    assert gather_call(None, None, None, 0, None, fake, None, 1, None, fake, need0) == kmws.ERR_NOT_SUPPORTED
    assert unpack_call(fake, fake, N, kmws.SERVER, fake, fake, fake, fake, None, 1, fake, fake, need) == \
        kmws.ERR_NOT_SUPPORTED
    assert unpack_call(None, None, 0, kmws.CLIENT, None, None, None, fake, None, 1, None, fake, need0) == \
        kmws.ERR_NOT_SUPPORTED
