"""Reference for kmws_utf8_validate: a table-driven UTF-8 decoder written from
RFC 3629 section 4, the message rules of include/kmws_gpu.h, and the seeded
generators the tests share.  Pure Python; tests/test_utf8_ref.py pins it
against bytes.decode and a brute-force search before anything trusts it."""
from __future__ import annotations

import random
from typing import List, Optional, Sequence, Tuple

NOT_TEXT, OK, BAD, AFTER_BAD = 0, 1, 2, 3

# RFC 3629 section 4, UTF8-1 .. UTF8-4: lead range -> the ranges of its continuations
_SYNTAX = [
    (0x00, 0x7F, ()),
    (0xC2, 0xDF, ((0x80, 0xBF),)),
    (0xE0, 0xE0, ((0xA0, 0xBF), (0x80, 0xBF))),
    (0xE1, 0xEC, ((0x80, 0xBF), (0x80, 0xBF))),
    (0xED, 0xED, ((0x80, 0x9F), (0x80, 0xBF))),
    (0xEE, 0xEF, ((0x80, 0xBF), (0x80, 0xBF))),
    (0xF0, 0xF0, ((0x90, 0xBF), (0x80, 0xBF), (0x80, 0xBF))),
    (0xF1, 0xF3, ((0x80, 0xBF), (0x80, 0xBF), (0x80, 0xBF))),
    (0xF4, 0xF4, ((0x80, 0x8F), (0x80, 0xBF), (0x80, 0xBF))),
]
_LEAD: List[Optional[tuple]] = [None] * 256
for _lo, _hi, _rest in _SYNTAX:
    for _b in range(_lo, _hi + 1):
        _LEAD[_b] = _rest

# Decoder state: the ranges the next bytes must fall in (() = between code points).
START: tuple = ()


def step(pending: tuple, b: int) -> Optional[tuple]:
    """State after byte b, or None when b cannot follow."""
    if pending:
        lo, hi = pending[0]
        return pending[1:] if lo <= b <= hi else None
    return _LEAD[b]


def first_bad(data: bytes, pending: tuple = START) -> Tuple[Optional[int], tuple]:
    """(index of the first byte at which data stops being a prefix of a
    well-formed string, or None; the decoder state after the last good byte)."""
    for i, b in enumerate(data):
        nxt = step(pending, b)
        if nxt is None:
            return i, pending
        pending = nxt
    return None, pending


def valid(data: bytes) -> bool:
    i, pending = first_bad(data)
    return i is None and not pending


# ---- message rules ----

class StreamState:
    """One stream between frames: the open message, if any."""

    def __init__(self):
        self.open = False
        self.checked = False
        self.bad = False
        self.pending: tuple = START

    def copy(self) -> "StreamState":
        s = StreamState()
        s.open, s.checked, s.bad, s.pending = self.open, self.checked, self.bad, self.pending
        return s


def validate_stream(frames: Sequence[Tuple[int, bytes]], state: Optional[StreamState] = None):
    """frames: (header byte 0, plain payload) in wire order -> (per-frame
    results, the state after the last frame)."""
    st = state.copy() if state is not None else StreamState()
    out = []
    for b0, payload in frames:
        op, fin, rsv1 = b0 & 0x0F, b0 & 0x80, b0 & 0x40
        if op >= 8:
            out.append(NOT_TEXT)
            continue
        if op != 0:
            st.open, st.checked, st.bad, st.pending = True, op == 1 and not rsv1, False, START
        elif not st.open:
            out.append(NOT_TEXT)
            continue
        if not st.checked:
            out.append(NOT_TEXT)
        elif st.bad:
            out.append(AFTER_BAD)
        else:
            i, st.pending = first_bad(payload, st.pending)
            if i is not None or (fin and st.pending):
                st.bad = True
                out.append(BAD)
            else:
                out.append(OK)
        if fin:
            st.open, st.checked, st.bad, st.pending = False, False, False, START
    return out, st


# ---- generators ----

_RANGES = {1: [(0x20, 0x7E)], 2: [(0x80, 0x7FF)], 3: [(0x800, 0xD7FF), (0xE000, 0xFFFF)],
           4: [(0x10000, 0x10FFFF)]}


def text(rng: random.Random, nbytes: int, widths: Sequence[int] = (1, 2, 3, 4)) -> bytes:
    """Exactly nbytes of well-formed UTF-8, code point widths drawn from `widths`
    (the tail is filled with narrower code points where a wide one does not fit)."""
    out = bytearray()
    while len(out) < nbytes:
        w = rng.choice(widths)
        w = min(w, nbytes - len(out))
        lo, hi = rng.choice(_RANGES[w])
        out += chr(rng.randint(lo, hi)).encode("utf-8")
    assert len(out) == nbytes
    return bytes(out)


class TextPool:
    """A pool of mixed-width text generated once; take() cuts well-formed pieces
    of an exact size out of it (much faster than text() per message)."""

    def __init__(self, rng: random.Random, size: int = 1 << 18, widths: Sequence[int] = (1, 2, 3, 4)):
        self.data = text(rng, size, widths)
        self.starts = [i for i, b in enumerate(self.data) if (b & 0xC0) != 0x80]

    def take(self, rng: random.Random, n: int) -> bytes:
        if n == 0:
            return b""
        out = bytearray()
        while len(out) < n:
            s = self.starts[rng.randrange(len(self.starts))]
            e = min(s + n - len(out), len(self.data))
            while e < len(self.data) and e > s and (self.data[e] & 0xC0) == 0x80:
                e -= 1
            out += self.data[s:e] if e > s else b"x"  # (the pool's end is a code point boundary)
        return bytes(out)


def fragment(rng: random.Random, payload: bytes, max_parts: int = 5, allow_empty: bool = True) -> List[bytes]:
    """payload cut at random byte positions (code points may straddle)."""
    k = rng.randint(1, max_parts)
    cuts = sorted(rng.randint(0, len(payload)) for _ in range(k - 1))
    if not allow_empty:
        cuts = sorted(set(c for c in cuts if 0 < c < len(payload)))
    edges = [0] + cuts + [len(payload)]
    return [payload[a:b] for a, b in zip(edges, edges[1:])]


def message(parts: Sequence[bytes], opcode: int = 1, rsv1: bool = False, fin: bool = True) -> List[Tuple[int, bytes]]:
    """The frames of one message: a head with `opcode`, then CONTINUE frames."""
    frames = []
    for k, p in enumerate(parts):
        b0 = (opcode if k == 0 else 0) | (0x40 if rsv1 and k == 0 else 0)
        if fin and k == len(parts) - 1:
            b0 |= 0x80
        frames.append((b0, p))
    return frames


def random_stream(rng: random.Random, nmsgs: int, max_len: int = 600, p_corrupt: float = 1 / 3,
                  p_binary: float = 1 / 6, p_rsv1: float = 0.08, p_ctrl: float = 0.15,
                  max_parts: int = 5) -> List[Tuple[int, bytes]]:
    """A stream of fragmented messages: text (one byte corrupted with p_corrupt),
    binary and RSV1 ones, control frames with non-UTF-8 payloads in between."""
    frames: List[Tuple[int, bytes]] = []
    for _ in range(nmsgs):
        n = rng.choice([0, 1, 2, 3, 4, 5, 17, 64]) if rng.random() < 0.3 else rng.randint(1, max_len)
        body = bytearray(text(rng, n))
        r = rng.random()
        op, rsv1 = 1, False
        if r < p_binary:
            op, body = 2, bytearray(rng.randrange(256) for _ in range(n))
        elif r < p_binary + p_rsv1:
            rsv1, body = True, bytearray(rng.randrange(256) for _ in range(n))
        elif r < p_binary + p_rsv1 + p_corrupt and n:
            body[rng.randrange(n)] = rng.choice([0xFF, 0xC0, 0x80, 0xED, 0xF5, 0xE0])
        for fr in message(fragment(rng, bytes(body), max_parts), op, rsv1):
            if rng.random() < p_ctrl:
                frames.append((0x80 | rng.choice([9, 10]), bytes(rng.randrange(0x80, 0x100)
                                                                  for _ in range(rng.randint(0, 9)))))
            frames.append(fr)
    return frames
