"""kmws_decoder_set_utf8_check without a GPU: the header still compiles as
plain C with the kmws_frame_utf8 macro; the entry is a no-op on NULL; a
CLIENT-mode decoder fed unmasked EMPTY frames needs no GPU work and still gives
the verdicts (an empty FIN text frame is a whole, well-formed message; rule (b)
on an empty FIN frame is decided by the host state alone); with the check off
kmws_frame_hdr.reserved stays 0."""
import os
import subprocess

from kuma_amd import kmws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_header_is_plain_c_with_the_macro(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "kmws_gpu.h"\n'
                   'int main(void){ kmws_frame_hdr h; h.reserved = KMWS_UTF8_BAD;\n'
                   '  kmws_decoder_set_utf8_check((kmws_decoder*)0, 1);\n'
                   '  return kmws_frame_utf8(&h) == KMWS_UTF8_BAD ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, "-fsyntax-only",
                           str(src)])


def test_null_decoder_is_a_no_op():
    assert kmws.lib().kmws_decoder_set_utf8_check(None, 1) is None
    assert kmws.lib().kmws_decoder_set_utf8_check(None, 0) is None


def test_frame_utf8_function_reads_reserved():
    h = kmws.FrameHdr()
    h.reserved = kmws.UTF8_AFTER_BAD
    assert kmws.lib().kmws_frame_utf8(h) == kmws.UTF8_AFTER_BAD
    assert kmws.lib().kmws_frame_utf8(None) == kmws.UTF8_NOT_TEXT


def _feed_empty_frames(check):
    """Unmasked empty frames into a CLIENT decoder: no payload, so no GPU work
    even where there is no device."""
    h = kmws.WSHandler(kmws.CLIENT)
    if check is not None:
        h.setUtf8Check(check)
    got = []
    h.setFrameCallback(lambda hdr, payload: got.append((hdr.opcode, hdr.fin, len(payload), hdr.utf8)))
    wire = bytes([0x81, 0x00,    # empty FIN text frame: a whole, well-formed message
                  0x89, 0x00,    # PING
                  0x82, 0x00,    # empty binary frame
                  0x01, 0x00,    # empty text head ...
                  0x8A, 0x00,    # PONG in between
                  0x00, 0x00,    # ... empty CONTINUE
                  0x80, 0x00,    # ... empty FIN: still a well-formed (empty) message
                  0x80, 0x00])   # CONTINUE with no open message
    assert h.handleData(wire) == kmws.WS_NOERR
    return got


def test_empty_frames_need_no_gpu_and_get_verdicts():
    got = _feed_empty_frames(True)
    assert [(g[0], g[1], g[2]) for g in got] == [(1, 1, 0), (9, 1, 0), (2, 1, 0), (1, 0, 0), (10, 1, 0), (0, 0, 0),
                                                  (0, 1, 0), (0, 1, 0)]
    assert [g[3] for g in got] == [kmws.UTF8_OK, kmws.UTF8_NOT_TEXT, kmws.UTF8_NOT_TEXT, kmws.UTF8_OK,
                                   kmws.UTF8_NOT_TEXT, kmws.UTF8_OK, kmws.UTF8_OK, kmws.UTF8_NOT_TEXT]


def test_check_off_leaves_reserved_zero():
    for check in (None, False):
        assert [g[3] for g in _feed_empty_frames(check)] == [0] * 8


def test_reset_clears_the_message_state():
    h = kmws.WSHandler(kmws.CLIENT)
    h.setUtf8Check(True)
    got = []
    h.setFrameCallback(lambda hdr, payload: got.append(hdr.utf8))
    assert h.handleData(bytes([0x01, 0x00])) == kmws.WS_NOERR          # an open text message
    h.reset()
    assert h.handleData(bytes([0x80, 0x00])) == kmws.WS_NOERR          # its CONTINUE: no open message any more
    assert got == [kmws.UTF8_OK, kmws.UTF8_NOT_TEXT]


def test_header_positional_construction_still_works():
    h = kmws.Header(1, 0, 0, 0, kmws.OP_TEXT, 0, b"\0\0\0\0", 5, 5, 0)
    assert h.utf8 == 0 and h.length == 5
