"""Sequential model of the protocol check (kmws_proto_check,
kmws_decoder_set_proto_check), written from RFC 6455 (5.2 opcodes and RSV bits,
5.4 fragmentation, 5.5 control frames, 5.5.1 / 7.4 the CLOSE body) as the issue
states the rule; it never calls the library.  Known answers typed by hand, the
seeded fuzz the GPU tests share, and helpers that lay streams out as a device
batch or as wire bytes.

A frame is Fr(b0, payload, err): b0 = header byte 0 (fin << 7 | rsv << 4 |
opcode), err = the parser's error byte.  Only a CLOSE frame's payload matters.
"""
import random
from collections import namedtuple

OK, RSV, OPCODE, CONTROL, CONTINUATION, INTERLEAVED = 0, 1, 2, 3, 4, 5
CLOSE_PAYLOAD, CLOSE_REASON, AFTER_CLOSE, HEADER, AFTER_FAIL = 6, 7, 8, 9, 10
NAMES = ["OK", "RSV", "OPCODE", "CONTROL", "CONTINUATION", "INTERLEAVED", "CLOSE_PAYLOAD", "CLOSE_REASON",
         "AFTER_CLOSE", "HEADER", "AFTER_FAIL"]
IDLE, OPEN, CLOSED, FAILED = 0, 1, 2, 3

Fr = namedtuple("Fr", "b0 payload err")


def fr(op, fin=1, rsv=0, payload=b"", err=0):
    """rsv: bits of 0x70."""
    return Fr((0x80 if fin else 0) | rsv | op, bytes(payload), err)


def close(code=None, reason=b"", fin=1, rsv=0):
    body = b"" if code is None else bytes([code >> 8, code & 0xFF]) + reason
    return fr(8, fin, rsv, body)


def code_ok(code):
    return 1000 <= code <= 1003 or 1007 <= code <= 1014 or 3000 <= code <= 4999


def local_class(f, rsv_allowed):
    op, fin, rsv, n = f.b0 & 15, f.b0 & 0x80, f.b0 & 0x70, len(f.payload)
    if f.err:
        return HEADER
    if rsv & ~(rsv_allowed if op in (1, 2) else 0):
        return RSV
    if 3 <= op <= 7 or 11 <= op <= 15:
        return OPCODE
    if op >= 8 and (not fin or n > 125):
        return CONTROL
    if op == 8:
        if n == 1 or (n >= 2 and not code_ok(f.payload[0] << 8 | f.payload[1])):
            return CLOSE_PAYLOAD
        try:
            f.payload[2:].decode("utf-8")  # strict: RFC 3629, and a string that ends inside a code point fails
        except UnicodeDecodeError:
            return CLOSE_REASON
    return OK


def judge(frames, rsv_allowed=0, state=IDLE):
    """-> (verdict per frame, state after)."""
    out = []
    for f in frames:
        op = f.b0 & 15
        if state == FAILED:
            out.append(AFTER_FAIL)
            continue
        if state == CLOSED:
            out.append(AFTER_CLOSE)
            continue
        loc = local_class(f, rsv_allowed)
        if loc:
            v = loc
        elif state == IDLE and op == 0:
            v = CONTINUATION
        elif state == OPEN and op in (1, 2):
            v = INTERLEAVED
        else:
            v = OK
        out.append(v)
        if v != OK:
            state = FAILED
        elif op == 8:
            state = CLOSED
        elif op < 8:
            state = IDLE if f.b0 & 0x80 else OPEN
    return out, state


T, B, C, PING, PONG = 1, 2, 0, 9, 10
R1, R2, R3 = 0x40, 0x20, 0x10

# (name, rsv_allowed, frames, verdicts typed by hand, state after typed by hand)
KNOWN = [
    ("text", 0, [fr(T)], [0], IDLE),
    ("binary_then_text", 0, [fr(B, payload=b"x" * 300), fr(T)], [0, 0], IDLE),
    ("three_fragments", 0, [fr(T, 0), fr(C, 0), fr(C, 1)], [0, 0, 0], IDLE),
    ("two_fragments_binary", 0, [fr(B, 0), fr(C, 1)], [0, 0], IDLE),
    ("ping_inside_message", 0, [fr(T, 0), fr(PING, payload=b"p"), fr(C, 1)], [0, 0, 0], IDLE),
    ("pong_and_ping_inside_message", 0, [fr(T, 0), fr(PONG), fr(C, 0), fr(PING), fr(C, 1), fr(T)], [0] * 6, IDLE),
    ("left_open", 0, [fr(T, 0), fr(C, 0)], [0, 0], OPEN),
    ("continue_first", 0, [fr(C, 1), fr(T)], [4, 10], FAILED),
    ("continue_first_no_fin", 0, [fr(C, 0)], [4], FAILED),
    ("continue_after_finished_message", 0, [fr(T), fr(C, 1)], [0, 4], FAILED),
    ("continue_after_ping_only", 0, [fr(PING), fr(C, 1)], [0, 4], FAILED),
    ("text_text", 0, [fr(T, 0), fr(T, 1)], [0, 5], FAILED),
    ("text_binary_no_fin", 0, [fr(T, 0), fr(B, 0), fr(C, 1)], [0, 5, 10], FAILED),
    ("text_ping_text", 0, [fr(T, 0), fr(PING), fr(T, 1)], [0, 0, 5], FAILED),
    ("ping_without_fin", 0, [fr(PING, 0)], [3], FAILED),
    ("pong_of_126_bytes", 0, [fr(PONG, payload=b"\0" * 126)], [3], FAILED),
    ("pong_of_125_bytes", 0, [fr(PONG, payload=b"\0" * 125)], [0], IDLE),
    ("opcode_3", 0, [fr(3)], [2], FAILED),
    ("opcode_7_no_fin", 0, [fr(7, 0)], [2], FAILED),
    ("opcode_11", 0, [fr(11)], [2], FAILED),
    ("opcode_15_long_no_fin", 0, [fr(15, 0, payload=b"\0" * 200)], [2], FAILED),
    ("rsv1_head_not_negotiated", 0, [fr(T, rsv=R1)], [1], FAILED),
    ("rsv1_head_negotiated", R1, [fr(T, rsv=R1), fr(B, 0, rsv=R1), fr(C, 1)], [0, 0, 0], IDLE),
    ("rsv2_head_rsv1_negotiated", R1, [fr(T, rsv=R2)], [1], FAILED),
    ("rsv12_head_rsv1_negotiated", R1, [fr(B, rsv=R1 | R2)], [1], FAILED),
    ("rsv3_head_all_negotiated", 0x70, [fr(B, rsv=R1 | R2 | R3)], [0], IDLE),
    ("rsv1_continue_negotiated", R1, [fr(T, 0, rsv=R1), fr(C, 1, rsv=R1)], [0, 1], FAILED),
    ("rsv1_ping_negotiated", R1, [fr(PING, rsv=R1)], [1], FAILED),
    ("rsv1_close_negotiated", R1, [close(1000, rsv=R1)], [1], FAILED),
    ("rsv_before_opcode", 0, [fr(3, rsv=R3)], [1], FAILED),
    ("close_empty", 0, [close()], [0], CLOSED),
    ("close_one_byte", 0, [fr(8, payload=b"\x03")], [6], FAILED),
    ("close_two_bytes", 0, [close(1000)], [0], CLOSED),
    ("close_three_bytes", 0, [close(1000, b"a")], [0], CLOSED),
    ("close_125_bytes", 0, [close(1001, b"a" * 123)], [0], CLOSED),
    ("close_125_bytes_multibyte", 0, [close(1001, "€".encode() * 41)], [0], CLOSED),
    ("close_126_bytes", 0, [close(1001, b"a" * 124)], [3], FAILED),
    ("close_without_fin_bad_code", 0, [close(999, fin=0)], [3], FAILED),
    ("close_999", 0, [close(999)], [6], FAILED),
    ("close_1000", 0, [close(1000)], [0], CLOSED),
    ("close_1003", 0, [close(1003)], [0], CLOSED),
    ("close_1004", 0, [close(1004)], [6], FAILED),
    ("close_1006", 0, [close(1006)], [6], FAILED),
    ("close_1007", 0, [close(1007)], [0], CLOSED),
    ("close_1014", 0, [close(1014)], [0], CLOSED),
    ("close_1015", 0, [close(1015)], [6], FAILED),
    ("close_2999", 0, [close(2999)], [6], FAILED),
    ("close_3000", 0, [close(3000)], [0], CLOSED),
    ("close_4999", 0, [close(4999, b"bye")], [0], CLOSED),
    ("close_5000", 0, [close(5000)], [6], FAILED),
    ("close_0", 0, [close(0)], [6], FAILED),
    ("close_65535", 0, [close(65535)], [6], FAILED),
    ("close_bad_code_and_bad_reason", 0, [close(1005, b"\xff")], [6], FAILED),
    ("close_reason_ends_inside_code_point", 0, [close(1000, b"ok\xe2\x82")], [7], FAILED),
    ("close_reason_lead_byte_only", 0, [close(1000, b"\xf0")], [7], FAILED),
    ("close_reason_bare_continuation", 0, [close(1000, b"\x80")], [7], FAILED),
    ("close_reason_surrogate", 0, [close(1000, b"\xed\xa0\x80")], [7], FAILED),
    ("close_reason_overlong", 0, [close(1000, b"a\xc0\xaf")], [7], FAILED),
    ("close_reason_bad_at_byte_125", 0, [close(1000, b"a" * 122 + b"\xc3")], [7], FAILED),
    ("close_reason_four_byte_code_point", 0, [close(1000, b"\xf0\x9f\x98\x80")], [0], CLOSED),
    ("frame_after_close", 0, [close(1000), fr(T)], [0, 8], CLOSED),
    ("ping_and_close_after_close", 0, [close(), fr(PING), close(1000), fr(3)], [0, 8, 8, 8], CLOSED),
    ("close_inside_message", 0, [fr(T, 0), close(1001), fr(C, 1)], [0, 0, 8], CLOSED),
    ("frames_after_failure", 0, [fr(3), fr(T), close(1000), fr(PING)], [2, 10, 10, 10], FAILED),
    ("bad_close_then_frame", 0, [close(1005), fr(T)], [6, 10], FAILED),
    ("bad_reason_then_close", 0, [fr(B), close(1000, b"\xbf"), close(1000)], [0, 7, 10], FAILED),
    ("header_error", 0, [fr(T), fr(B, err=1), fr(T)], [0, 9, 10], FAILED),
    ("header_error_wins", 0, [fr(11, 0, rsv=R1, payload=b"\0" * 200, err=6)], [9], FAILED),
]


# ---- the seeded fuzz ----

DATA_LENS = (0, 1, 7, 125, 126, 300)


def _clean_message(rng, rsv_allowed, data_lens):
    op = rng.choice((T, B))
    rsv = R1 if (rsv_allowed & R1) and rng.random() < 0.2 else 0
    nfrag = rng.choice((1, 1, 1, 2, 3, 5))
    out = []
    for k in range(nfrag):
        out.append(Fr((0x80 if k == nfrag - 1 else 0) | (rsv if k == 0 else 0) | (op if k == 0 else C),
                      b"d" * rng.choice(data_lens), 0))
        if k < nfrag - 1 and rng.random() < 0.3:
            out.append(fr(rng.choice((PING, PONG)), payload=b"c" * rng.choice((0, 5, 125))))
    return out


def _good_close(rng):
    if rng.random() < 0.2:
        return close()
    reason = rng.choice((b"", b"bye", "grüß".encode(), "€".encode() * 41, b"a" * 123,
                         b"\xf0\x9f\x98\x80" * 30))
    return close(rng.choice((1000, 1001, 1003, 1007, 1011, 1014, 3000, 4000, 4999)), reason)


def _violation(rng, state_open, rsv_allowed):
    """A frame (or two) that draws `kind`, given the stream is IDLE or OPEN."""
    kind = rng.choice((RSV, OPCODE, CONTROL, CONTINUATION, INTERLEAVED, CLOSE_PAYLOAD, CLOSE_REASON, AFTER_CLOSE,
                       HEADER))
    if kind == RSV:
        return [rng.choice((fr(T if not state_open else C, rsv=R2), fr(PING, rsv=R1), fr(C, rsv=R1),
                            fr(B if not state_open else C, rsv=0x70 & ~rsv_allowed or R1)))]
    if kind == OPCODE:
        return [fr(rng.choice((3, 4, 5, 6, 7, 11, 12, 13, 14, 15)), rng.randrange(2))]
    if kind == CONTROL:
        return [rng.choice((fr(PING, 0), fr(PONG, payload=b"\0" * 126), close(1000, fin=0), close(1000, b"a" * 124)))]
    if kind == CONTINUATION:
        return ([] if not state_open else [fr(C, 1)]) + [fr(C, rng.randrange(2))]
    if kind == INTERLEAVED:
        return ([] if state_open else [fr(T, 0)]) + [fr(rng.choice((T, B)), rng.randrange(2))]
    if kind == CLOSE_PAYLOAD:
        return [rng.choice((fr(8, payload=b"\x03"), close(999), close(1004), close(1005), close(1006), close(1015),
                            close(2999), close(5000), close(1016, b"why")))]
    if kind == CLOSE_REASON:
        return [close(1000, rng.choice((b"\x80", b"ok\xe2\x82", b"\xed\xa0\x80", b"a" * 122 + b"\xc3", b"\xff",
                                        b"\xf4\x90\x80\x80")))]
    if kind == AFTER_CLOSE:
        return [_good_close(rng)]
    return [fr(rng.choice((T, B, C, PING, 8)), err=rng.choice((5, 6, 7)))]


def _junk(rng):
    return rng.choice((fr(T), fr(C, 0), fr(PING), close(1000), fr(3), fr(B, 0, rsv=R1), close(999), fr(T, err=7)))


def fuzz_streams(seed=20260, n_streams=2000, rsv_allowed=R1, data_lens=DATA_LENS):
    """n_streams streams of about 20 frames: clean ones (whole and fragmented
    messages, control frames between fragments, maybe left open, maybe ended by a
    valid CLOSE), and ones with one violation of a random kind after a clean
    prefix, followed by more frames.  data_lens: the payload lengths of data
    frames (the check never looks at those payloads)."""
    rng = random.Random(seed)
    streams = []
    for _ in range(n_streams):
        s = []
        for _ in range(rng.randrange(0, 13)):
            s += _clean_message(rng, rsv_allowed, data_lens)
        r = rng.random()
        if r < 0.15:  # left open
            s += [fr(rng.choice((T, B)), 0), fr(PING)]
        elif r < 0.30:
            s.append(_good_close(rng))
        elif r >= 0.45:
            state_open = bool(s) and rng.random() < 0.4
            if state_open:
                s += [fr(rng.choice((T, B)), 0)]
            s += _violation(rng, state_open, rsv_allowed)
            for _ in range(rng.randrange(1, 12)):
                s.append(_junk(rng))
        streams.append(s)
    return streams


# ---- layouts ----

def mask_bytes(data, key):
    """key: the 4 wire key bytes."""
    return bytes(b ^ key[j & 3] for j, b in enumerate(data))


def device_batch(streams, masked=False, key_of=None, align=0, pad_end=0):
    """-> dict(base bytes, off[], len[], key[], flags[], err[], stream_first[]).
    Only CLOSE payloads are laid out in base (each at an offset = align mod 16,
    behind 16 filler bytes); every other frame's descriptor points at offset 0
    with its real length, whatever the span -- the check must not read there.
    key_of(i) -> 4 key bytes of frame i (default: derived from i); masked: the
    bytes in base are masked with them.  pad_end: filler bytes after the last
    payload (0: the last CLOSE payload ends exactly at the span)."""
    base = bytearray()
    off, ln, key, flags, err, first = [], [], [], [], [], [0]
    i = 0
    for s in streams:
        for f in s:
            k = int.from_bytes(key_of(i), "little") if key_of else \
                ((i * 7 + 1) & 0xFF) | ((i * 13 + 5) & 0xFF) << 8 | ((i >> 3) & 0xFF) << 16 | 0xA5 << 24
            o = 0
            if (f.b0 & 15) == 8 and f.payload:
                base += b"\xee" * 16
                base += b"\xee" * ((align - len(base)) % 16)
                o = len(base)
                base += mask_bytes(f.payload, k.to_bytes(4, "little")) if masked else f.payload
            off.append(o)
            ln.append(len(f.payload))
            key.append(k)
            flags.append(f.b0 | 0x100)
            err.append(f.err)
            i += 1
        first.append(i)
    base += b"\xee" * pad_end
    return dict(base=bytes(base), off=off, len=ln, key=key, flags=flags, err=err, stream_first=first)


def wire_header(b0, n, key=None):
    m = 0x80 if key is not None else 0
    if n < 126:
        h = bytes([b0, m | n])
    elif n < 65536:
        h = bytes([b0, m | 126]) + n.to_bytes(2, "big")
    else:
        h = bytes([b0, m | 127]) + n.to_bytes(8, "big")
    return h + (key or b"")


def deliverable(frames):
    """The frames of a stream the host decoder delivers: it stops, as kuma does,
    at a header error, at a control frame without FIN or above 125 bytes, and
    after the first CLOSE."""
    out = []
    for f in frames:
        op = f.b0 & 15
        if f.err or (op >= 8 and (not f.b0 & 0x80 or len(f.payload) > 125)):
            break
        out.append(f)
        if op == 8:
            break
    return out


def wire_of(frames, key_of=None):
    """The frames as wire bytes; key_of(i) -> 4 key bytes: masked (client to server)."""
    w = bytearray()
    for i, f in enumerate(frames):
        k = key_of(i) if key_of else None
        w += wire_header(f.b0, len(f.payload), k)
        w += mask_bytes(f.payload, k) if k else f.payload
    return bytes(w)
