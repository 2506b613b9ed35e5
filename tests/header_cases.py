"""Deterministic header-rule cases for the device frame parse (`unpack_one` in
kuma_amd/csrc/kmws_frame_parse.hpp, inlined into kmws_unpack_headers,
kmws_unpack_unmask and kmws_unpack_gather) and for the two header-chain walks
(kmws_find_headers on the host, kmws_find_headers_streams on the device), with
the per-frame and per-stream expectations taken from the oracle decoder
(oracle.oracle.Decoder) alone.  Plain numpy: no torch, no GPU.

A corpus is one wire image holding hand-built header records -- most of them
not encodable by encodeFrameHeader -- separated by random gaps, every record
kind at every byte phase (header offset mod 16), so that each rule is read
through every funnel shift of the aligned-load path.  `expect` restates the
contract of kmws_unpack_headers (include/kmws_gpu.h) over the oracle;
`walk_expect` does the same for the walks.  tests/test_header_cases.py proves
the corpus's claims and runs the host walk; tests/test_gpu_headers.py runs the
device entries.
"""
import functools
import json
import os

import numpy as np

from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LEN = 10 * 1024 * 1024  # KMWS_MAX_FRAME_DATA_LENGTH (WSHandler.cpp:110)
CLIENT, SERVER = orc.CLIENT, orc.SERVER

LENGTH_SWEEP_B0 = (0x81, 0x82, 0x80, 0x02, 0x88, 0x89, 0x8A, 0x09)
PATTERN_ROOM = 300  # bytes that follow a 127-class pattern record before the next gap


# ------------------------------ header records ------------------------------
def p7(v):
    """Length form: the 7-bit length v (0..125) in byte 1."""
    return ("p", int(v))


def x16(v):
    """Length form: 126 in byte 1, then v as two big-endian bytes (any v)."""
    return ("x16", int(v))


def x64(v):
    """Length form: 127 in byte 1, then eight raw bytes (an int is written big-endian)."""
    raw = int(v).to_bytes(8, "big") if not isinstance(v, (bytes, str)) else (
        bytes.fromhex(v) if isinstance(v, str) else v)
    assert len(raw) == 8
    return ("x64", raw.hex())


def header_bytes(b0, mask, form, key=b""):
    """The raw header: byte 0, byte 1 = mask << 7 | class, the extended length, the key if masked."""
    kind, v = form
    m = 0x80 if mask else 0
    if kind == "p":
        assert 0 <= v <= 125
        out = bytes([b0, m | v])
    elif kind == "x16":
        out = bytes([b0, m | 126]) + int(v).to_bytes(2, "big")
    else:
        out = bytes([b0, m | 127]) + bytes.fromhex(v)
    if mask:
        assert len(key) == 4
        out += bytes(key)
    return out


def nominal_length(form):
    """What the length bytes say when read as a plain big-endian number (used
    only to decide how many payload bytes a record is given)."""
    kind, v = form
    return int(v) if kind != "x64" else int.from_bytes(bytes.fromhex(v), "big")


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")) as f:
        return json.load(f)


def quirk127_patterns():
    """The eight length bytes of every quirk127_* vector of the golden set."""
    return [c["name"].split("_", 1)[1] for c in _golden()["decode"] if c["name"].startswith("quirk127_")]


def x64_patterns():
    """127-class quirk and rejection patterns: the golden quirk127_* set, bit 63
    from byte 0, sign extension from byte 4, and a single non-zero byte in each
    of the eight positions (0x01: through the shift aliasing the positions give
    2^24, 65536, 256, 1, 2^24, 65536, 256, 1)."""
    pats = list(quirk127_patterns()) + ["8000000000000000", "0000000080000000"]
    pats += [(b"\0" * k + b"\x01" + b"\0" * (7 - k)).hex() for k in range(8)]
    seen, out = set(), []
    for p in pats:
        # the cap and cap + 1 written plainly are the boundary forms below
        if p not in seen and int(p, 16) not in (MAX_LEN, MAX_LEN + 1):
            seen.add(p)
            out.append(p)
    return out


FLAG_SWEEP_FORMS = (p7(0), p7(5), p7(125), x16(126), x64(65536))
LENGTH_SWEEP_PLAIN = ([p7(0), p7(1), p7(125)] + [x16(v) for v in (0, 125, 126, 127, 65535)] +
                      [x64(v) for v in (0, 125, 65535, 65536, MAX_LEN, MAX_LEN + 1)])


def record_kinds():
    """Every (sweep, byte 0, mask, length form) of the two sweeps; pattern forms
    carry the tag "pat" so the layout gives them PATTERN_ROOM bytes."""
    kinds = []
    for b0 in range(256):
        for mask in (0, 1):
            for form in FLAG_SWEEP_FORMS:
                kinds.append(("flag", b0, mask, form, False))
    for b0 in LENGTH_SWEEP_B0:
        for mask in (0, 1):
            for form in LENGTH_SWEEP_PLAIN:
                kinds.append(("length", b0, mask, form, False))
            for pat in x64_patterns():
                if x64(pat) not in LENGTH_SWEEP_PLAIN:  # 2^16 in byte 5 is the plain 65536
                    kinds.append(("length", b0, mask, x64(pat), True))
    return kinds


def payload_room(kind, rng):
    """Bytes placed after a record's header before the next gap.  The payload is
    there in full (room = the nominal length) except: a pattern record gets
    PATTERN_ROOM bytes (a frame of at most that length is whole, gaps being
    legal; a longer one is cut off by the next record); nominal lengths above
    65536 get 0-40 bytes (cut off: err 5); and to keep the wire small the
    64 KiB payloads are present only in the length sweep behind a FIN-less or
    data byte 0 -- in the flag sweep and behind the control bytes 0x88 / 0x89 /
    0x8A / 0x09 they are cut off too."""
    sweep, b0, mask, form, is_pat = kind
    if is_pat:
        return PATTERN_ROOM
    L = nominal_length(form)
    full = L <= 127 or (L <= 65536 and sweep == "length" and (b0 & 0x0F) < 8)
    return L if full else int(rng.integers(0, 41))


def random_key(rng):
    """Four distinct non-zero key bytes."""
    return bytes((rng.permutation(255)[:4] + 1).astype(np.uint8))


class Corpus:
    """wire (uint8), hdr_off (int64, ascending), kind_id per record (-1: the
    records of the tail), kinds, mode."""

    def __init__(self, wire, hdr_off, kind_id, kinds, mode):
        self.wire, self.hdr_off, self.kind_id, self.kinds, self.mode = wire, hdr_off, kind_id, kinds, mode
        self.n = len(hdr_off)
        self.wire_len = len(wire)


@functools.lru_cache(maxsize=None)
def _sweep_image():
    """The part both corpora share: sixteen rounds over every record kind in a
    shuffled order; in round r kind k stands at phase (phase0[k] + r) mod 16,
    reached with a gap of 0-17 random bytes (the distance to that phase, plus
    16 at random when it is 0 or 1)."""
    rng = np.random.default_rng(0x4844_5231)
    kinds = record_kinds()
    phase0 = rng.integers(0, 16, size=len(kinds))
    parts, offs, ids = [], [], []
    cur = 0
    for r in range(16):
        for k in rng.permutation(len(kinds)):
            kind = kinds[k]
            gap = (int(phase0[k]) + r - cur) % 16
            if gap <= 1 and rng.integers(0, 2):
                gap += 16
            hdr = header_bytes(kind[1], kind[2], kind[3], random_key(rng) if kind[2] else b"")
            room = payload_room(kind, rng)
            parts.append(rng.integers(0, 256, size=gap, dtype=np.uint8))
            parts.append(np.frombuffer(hdr, np.uint8))
            parts.append(rng.integers(0, 256, size=room, dtype=np.uint8))
            offs.append(cur + gap)
            ids.append(k)
            cur += gap + len(hdr) + room
    return np.concatenate(parts), np.array(offs, np.int64), np.array(ids, np.int64), kinds


@functools.lru_cache(maxsize=None)
def corpus(mode):
    """The corpus of `mode`: the shared sweep image, then the frame at the cap
    and the one a byte above it, once each and complete, then three records the
    wire's end truncates (a payload, a 126-class payload inside the last 32
    bytes, a 127-class header cut inside its length bytes): the only way to
    err 1.  All masked for SERVER and unmasked for CLIENT (the form the mode
    accepts)."""
    body, offs, ids, kinds = _sweep_image()
    rng = np.random.default_rng(0x4844_5232 + mode)
    mask = 1 if mode == SERVER else 0
    parts, tail_offs = [body], []
    cur = len(body)
    for L in (MAX_LEN, MAX_LEN + 1):
        gap = int(rng.integers(0, 18))
        hdr = header_bytes(0x82, mask, x64(L), random_key(rng) if mask else b"")
        parts += [rng.integers(0, 256, size=gap, dtype=np.uint8), np.frombuffer(hdr, np.uint8),
                  rng.integers(0, 256, size=L, dtype=np.uint8)]
        tail_offs.append(cur + gap)
        cur += gap + len(hdr) + L
    for form, keep, room in ((x64(65536), 14, 20), (x16(300), 8, 10), (x64(70000), 5, 0)):
        gap = int(rng.integers(0, 18))
        hdr = header_bytes(0x82, mask, form, random_key(rng) if mask else b"")[:keep]
        parts += [rng.integers(0, 256, size=gap, dtype=np.uint8), np.frombuffer(hdr, np.uint8),
                  rng.integers(0, 256, size=room, dtype=np.uint8)]
        tail_offs.append(cur + gap)
        cur += gap + len(hdr) + room
    wire = np.concatenate(parts)
    return Corpus(wire, np.concatenate([offs, np.array(tail_offs, np.int64)]),
                  np.concatenate([ids, np.full(len(tail_offs), -1, np.int64)]), kinds, mode)


# ------------------------------ per-frame model ------------------------------
def _piece(wire, a, b):
    """A private copy of wire[a:b] (the oracle unmasks a whole frame in the buffer it is fed)."""
    return bytearray(wire[a:b])


def expect_full(wire, wire_len, hdr_off, f, mode, decoder=orc.Decoder):
    """(err, off, len, key, flags, payload): the contract of kmws_unpack_headers
    for frame f, from the decoder alone (payload: its unmasked bytes of a good
    frame, else b"").  decoder: the oracle's Decoder class, or the built
    reference's (oracle.reference().Decoder)."""
    h = int(hdr_off[f])
    nxt = int(hdr_off[f + 1]) if f + 1 < len(hdr_off) else int(wire_len)
    flags = (int(wire[h]) | ((int(wire[h + 1]) >> 7) << 8)) if h + 2 <= wire_len else 0
    d = decoder(mode)
    d.destroy_on = 0  # stop at the first delivered frame
    # the bytes from h to the wire's end, fed to one decoder in pieces: up to the
    # next header first, more only while it asks for more
    pos, end = h, max(h, min(nxt, wire_len))
    while True:
        ret = d.feed(_piece(wire, pos, end))
        if d.frames or ret not in (0, 1) or end >= wire_len:
            break
        pos, end = end, min(int(wire_len), end + max(4096, 2 * (end - h)))
    if d.frames:
        fr = d.frames[0]
        hl = 2 + (2 if fr.plen == 126 else 8 if fr.plen == 127 else 0) + (4 if fr.mask else 0)
        if h + hl + fr.length > nxt:
            return 5, h, 0, 0, flags, b""
        key = int.from_bytes(fr.maskey, "little") if fr.mask else 0
        return 0, h + hl, int(fr.length), key, flags, fr.payload
    if ret in (6, 7):
        return ret, h, 0, 0, flags, b""
    if ret in (0, 1):
        return 1, h, 0, 0, flags, b""
    raise AssertionError(f"{decoder.__name__} returned {ret} for the frame at {h}")


def expect(wire, wire_len, hdr_off, f, mode, decoder=orc.Decoder):
    """(err, off, len, key, flags) of frame f: see expect_full."""
    return expect_full(wire, wire_len, hdr_off, f, mode, decoder)[:5]


class Expected:
    """expect over a whole batch as arrays, and the good frames' payloads."""

    def __init__(self, wire, wire_len, hdr_off, mode, decoder=orc.Decoder):
        n = len(hdr_off)
        self.err = np.zeros(n, np.uint8)
        self.off = np.zeros(n, np.int64)
        self.len = np.zeros(n, np.int64)
        self.key = np.zeros(n, np.int64)
        self.flags = np.zeros(n, np.int64)
        self.payload = [b""] * n
        for f in range(n):
            (self.err[f], self.off[f], self.len[f], self.key[f], self.flags[f],
             self.payload[f]) = expect_full(wire, wire_len, hdr_off, f, mode, decoder)

    def desc(self):
        """(n, 2) int64 as the device writes kmws_desc: off, len | key << 32."""
        return np.stack([self.off, (self.len | (self.key << 32)).astype(np.uint64).view(np.int64)], axis=1)


@functools.lru_cache(maxsize=None)
def corpus_expected(mode):
    c = corpus(mode)
    return Expected(c.wire, c.wire_len, c.hdr_off, mode)


# ------------------------------ walk model and streams ------------------------------
def walk_expect(stream, cap, decoder=orc.Decoder):
    """(offsets, consumed) the header-chain walks must give for one stream: the
    offsets of the frames a SERVER oracle delivers, one more if bytes remain,
    the oracle did not close and fewer than cap are recorded; consumed = the end
    of the last delivered frame among those recorded."""
    stream = bytes(stream)
    d = decoder(SERVER)
    ret = d.feed(stream) if stream else 0
    offs, ends, p = [], [], 0
    for fr in d.frames:
        offs.append(p)
        p += 2 + (2 if fr.plen == 126 else 8 if fr.plen == 127 else 0) + (4 if fr.mask else 0) + fr.length
        ends.append(p)
    rec = offs[:cap]
    if len(offs) < cap and p < len(stream) and ret != 8:
        rec.append(p)
    nd = min(len(offs), cap)
    return rec, (ends[nd - 1] if nd else 0)


WALK_CAPS = (1, 15, 16, 17, 32, 33, 100)
WALK_COUNTS = (15, 16, 17, 31, 32, 33)
_VALID_B0 = (0x81, 0x82, 0x01, 0x02, 0x00, 0x80, 0x89, 0x8A)


def _valid_frame(rng):
    """A frame a SERVER accepts: masked, data or FIN control, 7-bit or 126-class length."""
    b0 = _VALID_B0[int(rng.integers(0, len(_VALID_B0)))]
    L = int(rng.integers(0, 126))
    if b0 < 0x88 and rng.integers(0, 4) == 0:
        L = int(rng.integers(126, 400))
    form = p7(L) if L <= 125 else x16(L)
    return header_bytes(b0, 1, form, random_key(rng)) + rng.integers(0, 256, size=L, dtype=np.uint8).tobytes()


def _valid_frames(rng, n):
    return [_valid_frame(rng) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def walk_streams():
    """{name: bytes}: each special frame in the middle of a stream of 5 frames
    (a cut ends the stream), the one-byte and the empty stream, and the frame
    counts around the device walk's 16-offset buffer."""
    rng = np.random.default_rng(0x57414C4B)
    out = {}
    # a 14-byte header: masked, 127-class (a non-minimal length, which kuma accepts)
    big = header_bytes(0x82, 1, x64(9), random_key(rng)) + rng.integers(0, 256, size=9, dtype=np.uint8).tobytes()
    for k in range(len(big) + 1):
        pre = b"".join(_valid_frames(rng, 2))
        post = b"".join(_valid_frames(rng, 2)) if k == len(big) else b""
        out[f"cut_{k:02d}"] = pre + big[:k] + post
    specials = {
        "close": header_bytes(0x88, 1, p7(2), random_key(rng)) + b"\x03\xe8",
        "x16_0": header_bytes(0x82, 1, x16(0), random_key(rng)),
        "x16_125": header_bytes(0x82, 1, x16(125), random_key(rng)) + bytes(125),
        "x64_bit63": header_bytes(0x82, 1, x64("8000000000000000"), random_key(rng)),
        "x64_max_plus_1": header_bytes(0x82, 1, x64(MAX_LEN + 1), random_key(rng)),
    }
    for name, sp in specials.items():
        out[name] = b"".join(_valid_frames(rng, 2)) + sp + b"".join(_valid_frames(rng, 2))
    out["one_byte"] = b"\x81"
    out["empty"] = b""
    for n in WALK_COUNTS:
        out[f"count_{n}"] = b"".join(_valid_frames(rng, n))
    return out


def filler_stream(k):
    """A stream of k bytes (0..15) that only moves the next stream's phase:
    empty unmasked frames and, for odd k, one truncated byte."""
    return b"\x80\x00" * (k // 2) + (b"\x81" if k & 1 else b"")


def place_streams(items, n_streams=None):
    """items: [(stream bytes, start phase)].  Streams are contiguous in a wire,
    so a filler stream stands before each one but the first (whose phase comes
    from stream_off[0]).  Returns (wire bytes from offset 0, stream_off list,
    streams in stream order).  n_streams: pad with empty streams up to it."""
    streams, off = [], []
    first_phase = items[0][1] % 16
    parts = [bytes(first_phase)]
    cur = first_phase
    off.append(cur)
    for i, (s, ph) in enumerate(items):
        if i:
            fl = filler_stream((ph - cur) % 16)
            streams.append(fl)
            parts.append(fl)
            cur += len(fl)
            off.append(cur)
        assert cur % 16 == ph % 16
        streams.append(bytes(s))
        parts.append(bytes(s))
        cur += len(s)
        off.append(cur)
    while n_streams is not None and len(streams) < n_streams:
        streams.append(b"")
        off.append(cur)
    assert n_streams is None or len(streams) == n_streams
    return b"".join(parts), off, streams


# ------------------------------ tail sweep records ------------------------------
@functools.lru_cache(maxsize=None)
def tail_records():
    """[(name, mode, frame bytes, header bytes, WSError of the whole frame)]:
    one good frame per header length (payload 3 bytes; the two 126-class ones
    need the smallest length that class may carry, 126) and the error records,
    for the sweep that cuts the wire at every byte of each."""
    rng = np.random.default_rng(0x5441494C)
    pay = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()  # noqa: E731
    key = lambda: random_key(rng)  # noqa: E731
    recs = [
        ("hl2", CLIENT, header_bytes(0x82, 0, p7(3)), 3, 0),
        ("hl4", CLIENT, header_bytes(0x81, 0, x16(126)), 126, 0),
        ("hl6", SERVER, header_bytes(0x82, 1, p7(3), key()), 3, 0),
        ("hl8", SERVER, header_bytes(0x01, 1, x16(126), key()), 126, 0),
        ("hl10", CLIENT, header_bytes(0x82, 0, x64(3)), 3, 0),
        ("hl14", SERVER, header_bytes(0x82, 1, x64(3), key()), 3, 0),
        ("control_not_fin", SERVER, header_bytes(0x09, 1, p7(3), key()), 3, 7),
        ("control_plen_126", SERVER, header_bytes(0x89, 1, x16(126), key()), 3, 7),
        ("x16_125", SERVER, header_bytes(0x82, 1, x16(125), key()), 3, 6),
        ("x64_bit63", SERVER, header_bytes(0x82, 1, x64("8000000000000003"), key()), 3, 6),
        ("masked_in_client", CLIENT, header_bytes(0x82, 1, p7(3), key()), 3, 7),
        ("unmasked_in_server", SERVER, header_bytes(0x82, 0, p7(3)), 3, 7),
    ]
    return [(name, mode, hdr + pay(n), len(hdr), err) for name, mode, hdr, n, err in recs]


def tail_wire(frame, phase, cut, stride):
    """One row of the tail sweep: a 2-byte empty frame at 0 when the phase leaves
    room for it, filler up to `phase`, the first `cut` bytes of `frame`, then 0xFF
    up to `stride` (so a read past wire_len changes the answer).
    Returns (row, wire_len, hdr_off list)."""
    row = np.full(stride, 0xFF, np.uint8)
    row[:phase] = 0x5A
    offs = [phase]
    if phase >= 2:
        row[0:2] = (0x82, 0x00)  # unmasked and empty: both modes accept it
        offs = [0, phase]
    row[phase:phase + cut] = np.frombuffer(frame[:cut], np.uint8)
    assert phase + cut <= stride
    return row, phase + cut, offs
