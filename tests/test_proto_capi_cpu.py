"""The protocol check without a GPU: the symbols and their bindings, the
workspace size, kmws_proto_check's argument checks (before any device work, in
the documented order; KMWS_ERR_NOT_SUPPORTED without a device, never a CPU
fallback), and the host path end to end -- kmws_decoder_set_proto_check judges
on the host, so a CLIENT-mode handler fed unmasked streams needs no device:
verdicts per delivered frame against tests/proto_ref.py, everything else
identical to the same feed with the check off."""
import ctypes as C

import pytest

import proto_ref as pr
from kuma_amd import kmws


def test_symbols_are_exported_and_bound():
    L = kmws.lib()
    for name in ("kmws_proto_workspace_size", "kmws_proto_check", "kmws_decoder_set_proto_check",
                 "kmws_decoder_frame_proto"):
        assert name in kmws.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert L.kmws_proto_check.restype is C.c_int and len(L.kmws_proto_check.argtypes) == 16
    assert L.kmws_proto_workspace_size.restype is C.c_size_t
    assert (kmws.PROTO_OK, kmws.PROTO_AFTER_FAIL) == (0, 10)
    # NULL decoders: no-ops
    L.kmws_decoder_set_proto_check(None, 1, 0x40)
    assert L.kmws_decoder_frame_proto(None) == 0


def test_workspace_size_is_monotone_and_small():
    size = kmws.lib().kmws_proto_workspace_size
    ns = [0, 1, 1023, 1024, 1025, 65536, 1 << 20, (1 << 23) + 1, (1 << 31) - 1]
    streams = [0, 1, 2, 1023, 1024, 1 << 16, 1 << 24, (1 << 31) - 1]
    for k in streams:
        v = [size(n, k) for n in ns]
        assert v == sorted(v) and v[0] < v[-1]
    for n in ns:
        v = [size(n, k) for k in streams]
        assert v == sorted(v)  # it grows only where the streams need more blocks than the frames
        assert n >= 1 << 23 or v[0] < v[-1]
    # about 2 B per frame (whole blocks of 1024) plus 3 B per block
    assert size(1 << 23, 1 << 16) <= 2 * (1 << 23) + 3 * (1 << 13) + 64
    assert kmws.proto_workspace_size(100) == size(100, 1)


def test_check_rejects_bad_arguments_before_any_device_work():
    L = kmws.lib()
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(4096 + 8)
    need = L.kmws_proto_workspace_size(5, 1)
    v = L.kmws_proto_check
    inv = kmws.ERR_INVALID_PARAM
    #          base  span     descs flags err   n  masked rsv  first ns carries     out   ws    bytes stream
    assert v(fake, 1 << 16, None, fake, None, 5, 0, 0, None, 1, None, None, fake, fake, need, None) == inv
    assert v(fake, 1 << 16, fake, None, None, 5, 0, 0, None, 1, None, None, fake, fake, need, None) == inv
    assert v(fake, 1 << 16, fake, fake, None, 5, 0, 0, None, 1, None, None, None, fake, need, None) == inv
    assert v(fake, 1 << 16, fake, fake, None, 5, 0, 0, None, 1, None, None, fake, None, need, None) == inv
    assert v(None, 1 << 16, fake, fake, None, 5, 0, 0, None, 1, None, None, fake, fake, need, None) == inv
    assert v(odd, 1 << 16, fake, fake, None, 5, 0, 0, None, 1, None, None, fake, fake, need, None) == inv
    assert v(fake, 1 << 16, fake, fake, None, 1 << 31, 0, 0, None, 1, None, None, fake, fake, 1 << 40, None) == inv
    assert v(fake, 1 << 16, fake, fake, None, 5, 0, 0, fake, 1 << 31, None, None, fake, fake, 1 << 40, None) == inv
    # stream_first NULL needs n_streams == 1; no streams cannot hold frames
    assert v(fake, 1 << 16, fake, fake, None, 5, 0, 0, None, 2, None, None, fake, fake, need, None) == inv
    assert v(fake, 1 << 16, fake, fake, None, 5, 0, 0, fake, 0, None, None, fake, fake, need, None) == inv
    # rsv_allowed holds RSV bits only -- tested before the workspace size
    for rsv in (0x80, 0x0F, 0x01, 0x100, 0x71):
        assert v(fake, 1 << 16, fake, fake, None, 5, 0, rsv, None, 1, None, None, fake, fake, 0, None) == inv
    # every INVALID_PARAM comes before BUFFER_TOO_SMALL
    assert v(fake, 1 << 16, None, fake, None, 5, 0, 0, None, 1, None, None, fake, fake, 0, None) == inv
    assert v(fake, 1 << 16, fake, fake, None, 5, 0, 0x70, None, 1, None, None, fake, fake, need - 1, None) == \
        kmws.ERR_BUFFER_TOO_SMALL
    assert v(fake, 1 << 16, fake, fake, fake, 5, 1, 0x40, None, 1, None, None, fake, fake, 0, None) == \
        kmws.ERR_BUFFER_TOO_SMALL


def test_check_without_device_is_not_supported():
    L = kmws.lib()
    if L.kmws_device_count() > 0:
        pytest.skip("a device is present")
    fake = C.c_void_p(4096)
    need = L.kmws_proto_workspace_size(5, 1)
    assert L.kmws_proto_check(fake, 1 << 16, fake, fake, None, 5, 0, 0, None, 1, None, None, fake, fake, need,
                              None) == kmws.ERR_NOT_SUPPORTED
    assert L.kmws_proto_check(None, 0, None, None, None, 0, 0, 0, None, 1, None, None, None, None, 0, None) == \
        kmws.ERR_NOT_SUPPORTED


# ---- the host path, no GPU ----

def host_streams():
    """(name, rsv_allowed, frames): the model's known answers and 200 fuzz
    streams, each cut before its first header-error frame (a wire cannot carry
    the parser's verdict on itself)."""
    out = [(name, rsv, frames) for name, rsv, frames, _, _ in pr.KNOWN]
    fuzz = pr.fuzz_streams(seed=77, n_streams=200, data_lens=(0, 1, 2, 5, 126))
    out += [(f"fuzz{k}", pr.R1, s) for k, s in enumerate(fuzz)]
    cut = []
    for name, rsv, frames in out:
        k = next((i for i, f in enumerate(frames) if f.err), len(frames))
        cut.append((name, rsv, frames[:k]))
    return cut


def feed(wire, chunk, rsv_allowed, check):
    """-> (return codes, delivered frames as tuples, verdict per delivered frame,
    verdicts read outside callbacks)."""
    h = kmws.WSHandler(kmws.CLIENT)
    if check:
        h.set_proto_check(True, rsv_allowed)
    got, verdicts, outside = [], [], []

    def cb(hd, p):
        got.append((hd.fin, hd.rsv1, hd.rsv2, hd.rsv3, hd.opcode, hd.mask, hd.plen, hd.xpl64, hd.maskey, hd.length,
                    hd.utf8, p))
        verdicts.append(h.last_frame_proto())

    h.setFrameCallback(cb)
    rets = []
    outside.append(h.last_frame_proto())
    for i in range(0, max(len(wire), 1), chunk):
        rets.append(h.handleData(wire[i:i + chunk]))
        outside.append(h.last_frame_proto())
    return rets, got, verdicts, outside


@pytest.mark.parametrize("chunk", [1, 5, 64, 65536])
def test_host_path_matches_the_model_and_changes_nothing_else(chunk):
    streams = host_streams()
    assert len(streams) == len(pr.KNOWN) + 200
    seen = set()
    for name, rsv, frames in streams:
        wire = pr.wire_of(frames)
        rets, got, verdicts, outside = feed(wire, chunk, rsv, True)
        rets0, got0, verdicts0, outside0 = feed(wire, chunk, rsv, False)
        assert (rets, got) == (rets0, got0), name  # advisory: nothing else changes
        assert not any(verdicts0) and not any(outside0) and not any(outside), name
        delivered = pr.deliverable(frames)
        assert [(g[4], g[0], g[-1]) for g in got] == [(f.b0 & 15, f.b0 >> 7, f.payload) for f in delivered], name
        want = pr.judge(frames, rsv)[0][:len(delivered)]
        assert verdicts == want, name
        seen.update(want)
    # everything the decoder can deliver occurs: all but the three it stops at
    assert seen == set(range(11)) - {pr.CONTROL, pr.AFTER_CLOSE, pr.HEADER}


def test_reset_restores_idle_and_switching_off_clears():
    h = kmws.WSHandler(kmws.CLIENT)
    h.set_proto_check(True)
    verdicts = []
    h.setFrameCallback(lambda hd, p: verdicts.append(h.last_frame_proto()))
    opened = pr.wire_of([pr.fr(pr.T, 0)])
    cont = pr.wire_of([pr.fr(pr.C, 1)])
    assert h.handleData(opened) == kmws.WS_NOERR and h.handleData(cont) == kmws.WS_NOERR
    assert verdicts == [0, 0]
    h.handleData(opened)
    h.reset()  # IDLE again: the CONTINUE has no message
    h.handleData(cont)
    assert verdicts[2:] == [0, pr.CONTINUATION]
    h.handleData(cont)
    assert verdicts[4:] == [pr.AFTER_FAIL]
    h.reset()
    h.handleData(opened)
    assert verdicts[5:] == [0]
    h.set_proto_check(False)  # off: 0 for every frame
    h.handleData(opened)
    assert verdicts[6:] == [0]
    h.set_proto_check(True)  # on again: starts IDLE
    h.handleData(cont)
    assert verdicts[7:] == [pr.CONTINUATION]
    # rsv_allowed is taken at every call
    h.reset()
    h.handleData(pr.wire_of([pr.fr(pr.T, rsv=pr.R1)]))
    h.set_proto_check(True, pr.R1)
    h.reset()
    h.handleData(pr.wire_of([pr.fr(pr.T, rsv=pr.R1)]))
    assert verdicts[8:] == [pr.RSV, 0]
