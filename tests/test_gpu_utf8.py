"""kmws_utf8_validate on the device against tests/utf8_ref.py (pinned by
tests/test_utf8_ref.py): known answers, corruptions around every word / tile
boundary, code points straddling fragments, the unmask tests' frame layouts
masked and plain, streams with the carry between two calls, the contract, and a
seeded fuzz whose mix is checked on the reference's verdicts."""
import functools
import os
import random
import re

import numpy as np
import pytest

import utf8_ref as ref

T_, C_, B_, FIN, RSV1, PING = 1, 0, 2, 0x80, 0x40, 9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- helpers

class Batch:
    """Frames (header byte 0, plain payload) placed at offs[] in an arena of
    `total` bytes; gaps hold bytes >= 0x80 (headers, other data: never looked at)."""

    def __init__(self, frames, offs, total, seed=1):
        self.frames = list(frames)
        self.n = len(self.frames)
        self.offs = np.asarray(offs, dtype=np.int64).reshape(-1)
        self.lens = np.array([len(p) for _, p in self.frames], dtype=np.int64)
        self.total = int(total)
        rng = np.random.default_rng(seed)
        self.keys = rng.integers(0, 2**32, size=self.n, dtype=np.uint64).astype(np.uint32)
        self.keys[::17] = 0
        self.flags = np.array([b0 for b0, _ in self.frames], dtype=np.int64) | 0x100
        self.plain = rng.integers(0x80, 0x100, size=(self.total + 15) // 16 * 16, dtype=np.uint8)
        assert self.n == 0 or (self.offs[-1] + self.lens[-1] <= self.total)
        if self.disjoint():
            at, _ = self.payload_index()
            self.plain[at] = np.frombuffer(b"".join(p for _, p in self.frames), dtype=np.uint8)
        else:
            for (_, p), o in zip(self.frames, self.offs):
                if p:
                    self.plain[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)

    def disjoint(self):
        """Few payload bytes, in ascending order without overlap (a test may move
        offs afterwards): one indexed pass serves.  Else frame by frame."""
        return int(self.lens.sum()) <= 1 << 22 and bool((self.offs[1:] >= self.offs[:-1] + self.lens[:-1]).all())

    def payload_index(self):
        """Per payload byte, frame after frame: its arena index and its position in its frame."""
        start = np.cumsum(self.lens) - self.lens
        within = np.arange(int(self.lens.sum()), dtype=np.int64) - np.repeat(start, self.lens)
        return np.repeat(self.offs, self.lens) + within, within

    def masked(self):
        buf = self.plain.copy()
        if self.disjoint():  # one pass over all payload bytes: a key's byte j & 3 on a frame's byte j
            at, within = self.payload_index()
            shift = ((within & 3) * 8).astype(np.uint32)
            buf[at] ^= ((np.repeat(self.keys, self.lens) >> shift) & np.uint32(0xFF)).astype(np.uint8)
            return buf
        for o, L, k in zip(self.offs, self.lens, self.keys):
            if L:
                kb = np.frombuffer(np.uint32(k).tobytes(), dtype=np.uint8)
                buf[o:o + L] ^= np.tile(kb, L // 4 + 1)[:L]
        return buf


def packed_offsets(lens, rng, first=None):
    """Payloads back to back behind 2..14-byte gaps (headers)."""
    offs, pos = [], 0
    for i, L in enumerate(lens):
        pos += rng.randint(2, 14) if (first is None or i) else first
        offs.append(pos)
        pos += L
    return offs, pos + 5


def run_gpu(batch, masked=False, stream_first=None, carry_in=None, lo=0, hi=None, keep=None):
    """Validates frames [lo, hi) of the batch; returns (out, carry_out, status)."""
    import torch as T
    from kuma_amd import kmws
    hi = batch.n if hi is None else hi
    n = hi - lo
    buf = batch.masked() if masked else batch.plain
    base = T.from_numpy(buf).cuda()
    descs = kmws.make_descs(batch.offs[lo:hi], batch.lens[lo:hi], batch.keys[lo:hi].astype(np.int64))
    fl = T.from_numpy(batch.flags[lo:hi].astype(np.int16)).cuda()
    out = T.full((max(n, 1),), 0xEE, dtype=T.uint8, device="cuda")
    ns = 1 if stream_first is None else len(stream_first) - 1
    sf = None if stream_first is None else T.tensor(list(stream_first), dtype=T.int32, device="cuda")
    ci = None if carry_in is None else T.from_numpy(np.ascontiguousarray(carry_in, dtype=np.uint8)).cuda()
    co = T.full((max(ns, 1), 8), 0xEE, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(kmws.utf8_workspace_size(batch.total, n, ns))
    kmws.utf8_validate(base, descs, fl, out, ws, span=batch.total, masked=masked, stream_first=sf, carry_in=ci,
                       carry_out=co)
    status = ws.status() if n else 0
    assert np.array_equal(base.cpu().numpy(), buf), "the payload was written"
    if keep is not None:
        keep.update(base=base, descs=descs, fl=fl, out=out, ws=ws)
    return out.cpu().numpy()[:n], co.cpu().numpy()[:ns], status


def want(frames):
    return np.array(ref.validate_stream(frames)[0], dtype=np.uint8)


def check(batch, expect=None, both=True):
    expect = want(batch.frames) if expect is None else np.asarray(expect, dtype=np.uint8)
    res = {}
    for m in ((False, True) if both else (False,)):
        out, _, st = run_gpu(batch, masked=m)
        assert st == 0
        bad = np.nonzero(out != expect)[0]
        assert bad.size == 0, (m, bad[:10], out[bad[:10]], expect[bad[:10]])
        res[m] = out
    return expect


# ---------------------------------------------------------------- known answers

KNOWN = [("κόσμε".encode(), True)] + \
    [(chr(c).encode(), True) for c in (0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x10FFFF)] + \
    [(bytes.fromhex(h), False) for h in ("C080", "E08080", "F0808080", "EDA080", "EDBFBF", "F4908080", "80",
                                         "E282", "FF")]


@pytest.mark.gpu
def test_known_answers():
    frames, expect = [], []
    for data, ok in KNOWN:
        assert ref.valid(data) == ok
        frames += [(T_ | FIN, data), (B_ | FIN, data), (T_ | FIN | RSV1, data)]
        expect += [ref.OK if ok else ref.BAD, ref.NOT_TEXT, ref.NOT_TEXT]
    offs, total = packed_offsets([len(p) for _, p in frames], random.Random(1))
    b = Batch(frames, offs, total)
    assert list(want(frames)) == expect
    check(b, expect)


# ---------------------------------------------------------------- boundary sweep

SWEEP_LEN = 40 * 1024


@functools.lru_cache(maxsize=None)
def sweep_text():
    data = ref.text(random.Random(40), SWEEP_LEN)
    assert ref.valid(data)
    return data, np.frombuffer(data, dtype=np.uint8)


# (unit, how many of its multiples from the frame start on): the four boundary classes
SWEEP_CLASSES = ((16, 4), (1024, 40), (4096, 10), (16384, 3))


def sweep_copies(off):
    """The corruptions of the copy at arena offset off: (class unit, p, new byte)
    with off + p within +-4 bytes of a multiple of the unit."""
    data, arr = sweep_text()
    seen, res = set(), []
    for unit, count in SWEEP_CLASSES:
        m0 = (off + unit - 1) // unit * unit
        for k in range(count):
            for dlt in range(-4, 5):
                p = m0 + k * unit + dlt - off
                if not 0 <= p < SWEEP_LEN:
                    continue
                if (unit, p, 0) not in seen:
                    seen.add((unit, p, 0))
                    res.append((unit, p, 0xFF))
                width = 2 if 0xC2 <= arr[p] <= 0xDF else 3 if 0xE0 <= arr[p] <= 0xEF else 4 if arr[p] >= 0xF0 else 0
                if width and p + width <= SWEEP_LEN and (unit, p, 1) not in seen:
                    seen.add((unit, p, 1))
                    res.append((unit, p + width - 1, 0x61))  # truncated: its last continuation becomes "a"
    return res


def sweep_verdict(copy, p):
    """The reference on one corrupted copy.  The pristine text is well-formed
    (checked once), so the bytes before the last code point boundary at least 4
    bytes ahead of p are a whole number of code points and the decoder is
    between code points there: the reference runs from that boundary."""
    b = max(p - 4, 0)
    while (copy[b] & 0xC0) == 0x80:
        b -= 1
    i, pending = ref.first_bad(bytes(copy[b:]))
    return ref.BAD if (i is not None or pending) else ref.OK


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["covered64k", "packed"])
@pytest.mark.parametrize("o", range(16))
def test_boundary_sweep(o, aligned):
    data, arr = sweep_text()
    rng = random.Random(100 + o)
    # place the copies: the corruptions of a copy depend on where it lies
    if aligned:  # every copy at o past a 64 KiB edge: one list serves all
        plan = [None] + sweep_copies(o)
        copies = [(j * 65536 + o, c) for j, c in enumerate(plan)]
    else:        # packed: each copy takes the j-th corruption of its own offset's list
        copies, pos = [(o, None)], o + SWEEP_LEN
        for j in range(len(sweep_copies(o))):
            off = pos + rng.randint(2, 14)
            cands = sweep_copies(off)
            copies.append((off, cands[j % len(cands)]))
            pos = off + SWEEP_LEN
    total = copies[-1][0] + SWEEP_LEN + 7
    b = Batch([(T_ | FIN, data)] * len(copies), [c[0] for c in copies], total)
    expect, classes = [], {}
    for off, c in copies:
        if c is None:
            expect.append(ref.OK)
            continue
        unit, p, newb = c
        b.plain[off + p] = newb
        expect.append(sweep_verdict(b.plain[off:off + SWEEP_LEN], p))
        classes[unit] = classes.get(unit, 0) + 1
    assert expect[0] == ref.OK and all(e == ref.BAD for e in expect[1:])
    assert all(classes.get(u, 0) >= 1 for u, _ in SWEEP_CLASSES), classes
    # plain for every offset, masked for four of them (the key phase follows the offset mod 4)
    check(b, expect, both=o % 4 == 1)


# ---------------------------------------------------------------- fragment straddles

def straddle_frames(rng):
    unit = "a€😀".encode()  # 1 + 3 + 4 bytes
    frames = []
    noise = lambda: bytes(rng.randrange(0x80, 0x100) for _ in range(rng.randint(1, 9)))

    def cut_message(body, at, cuts, fin_empty=False, head=T_):
        """body cut inside the sequence starting at `at` after cuts[] bytes of it,
        empty CONTINUE frames and a PING between the fragments."""
        edges = [0] + [at + c for c in cuts] + [len(body)]
        parts = [body[a:b] for a, b in zip(edges, edges[1:])]
        msg = []
        for k, p in enumerate(parts):
            msg.append(((head if k == 0 else C_), p))
            if k < len(parts) - 1:
                msg += [(C_, b""), (PING | FIN, noise()), (C_, b"")]
        if fin_empty:
            msg.append((C_ | FIN, b""))
        else:
            msg[-1] = (msg[-1][0] | FIN, msg[-1][1])
        frames.extend(msg)

    body = unit * 3
    emoji = len(unit) + 4  # the second unit's 4-byte code point
    for cuts in ([1], [2], [3], [1, 2, 3]):
        cut_message(body, emoji, cuts)
        cut_message(body, emoji, cuts, fin_empty=True)          # empty FIN after a complete code point: 1
        cut_message(body[:emoji + cuts[-1]], emoji, cuts[:-1], fin_empty=True)  # after an incomplete one: 2 on it
        cut_message(body, emoji, cuts, head=B_)                  # binary: all 0
    for seq, where in ((b"\xe0\x80\x80", "second"), (b"\xed\xa0\x80", "second"), (b"\xc0\x80", "first")):
        cut_message(b"ab" + seq + b"cd", 2, [1])
        frames.append((T_ | FIN, unit))                          # the next message is judged afresh
    return frames


@pytest.mark.gpu
def test_fragment_straddles():
    rng = random.Random(7)
    frames = straddle_frames(rng)
    expect = want(frames)
    # spot checks of the reference's own answers on this input
    assert set(expect) == {0, 1, 2, 3}
    empties_bad = [i for i, (b0, p) in enumerate(frames) if b0 == (C_ | FIN) and p == b"" and expect[i] == ref.BAD]
    empties_ok = [i for i, (b0, p) in enumerate(frames) if b0 == (C_ | FIN) and p == b"" and expect[i] == ref.OK]
    assert len(empties_bad) == 4 and len(empties_ok) == 4
    offs, total = packed_offsets([len(p) for _, p in frames], rng)
    check(Batch(frames, offs, total), expect)


def test_straddle_reference_answers():
    """CPU: the reference on the E0|80, ED|A0 and C0|80 cuts."""
    T, C = T_, C_
    run = lambda fr: ref.validate_stream(fr)[0]
    assert run([(T, b"ab\xe0"), (C | FIN, b"\x80\x80cd")]) == [1, 2]
    assert run([(T, b"ab\xed"), (C, b""), (C | FIN, b"\xa0\x80cd")]) == [1, 1, 2]
    assert run([(T, b"ab\xc0"), (C, b"\x80"), (C | FIN, b"cd")]) == [2, 3, 3]


# ---------------------------------------------------------------- layouts

def layout(kind, rng):
    """Frame offsets and lengths in the sense of tests/test_gpu_unmask.py::layout."""
    if kind == "packed_wire":  # payloads behind 2..14-byte headers: misaligned starts
        n = 150
        lens = rng.choice([0, 1, 7, 125, 126, 1000, 4096, 65535, 65536, 70001], size=n)
        hdr = np.where(lens <= 125, 2, np.where(lens <= 65535, 4, 10)) + 4
        wire = np.cumsum(np.concatenate([[0], hdr + lens]))
        offs = wire[:-1] + hdr
        total = int(wire[-1])
    elif kind == "tiny_many":  # > 256 frames per 16 KiB tile
        n = 20000
        lens = rng.integers(0, 21, size=n)
        gaps = rng.integers(0, 15, size=n)
        starts = np.cumsum(np.concatenate([[0], gaps + lens]))
        offs = starts[:-1] + gaps
        total = int(starts[-1])
    elif kind == "zero_len_runs":  # empty frames at equal offsets, adjacent frames, no gaps
        n = 3000
        lens = rng.choice([0, 0, 0, 1, 2, 3, 17, 300], size=n)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
        total = int(np.sum(lens)) + 3
    elif kind == "long_gaps":  # regions >= one tile: every header-gap size around a boundary
        n = 80
        gaps = rng.choice([0, 1, 2, 4, 8, 10, 14, 15, 16, 17, 31, 1024], size=n)
        lens = rng.integers(16384, 70000, size=n)
        offs = np.zeros(n, dtype=np.int64)
        pos = 0
        for i in range(n):
            pos += int(gaps[i])
            offs[i] = pos
            if i % 5 == 4:  # end on the next tile edge at least 16 KiB away
                lens[i] = (pos + 16384 + 16383) // 16384 * 16384 - pos
            pos += int(lens[i])
        total = pos + 9
    else:
        raise ValueError(kind)
    return np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64), total


def fill_messages(lens, seed, streams=None):
    """Messages over consecutive frames of the given lengths (so they are
    fragmented where the layout cuts): a third of the text messages get one
    corrupted byte, a sixth of all are binary, some RSV1; control frames and
    unfinished messages in between."""
    rng = random.Random(seed)
    pool = ref.TextPool(random.Random(seed + 1))
    frames, i, n = [], 0, len(lens)
    stops = set(streams or [])  # a message does not cross a stream start
    while i < n:
        if rng.random() < 0.1:
            frames.append((rng.choice([9, 10]) | FIN, bytes(rng.randrange(0x80, 0x100) for _ in range(int(lens[i])))))
            i += 1
            continue
        k = rng.randint(1, 5)
        j = i + 1
        while j < min(i + k, n) and j not in stops:
            j += 1
        size = int(sum(lens[i:j]))
        r = rng.random()
        op, rsv1 = T_, 0
        if r < 1 / 6:
            op, body = B_, bytearray(rng.randrange(256) for _ in range(size))
        elif r < 1 / 6 + 0.08:
            rsv1, body = RSV1, bytearray(rng.randrange(256) for _ in range(size))
        else:
            body = bytearray(pool.take(rng, size))
            if size and rng.random() < 1 / 3:
                body[rng.randrange(size)] = rng.choice([0xFF, 0xC0, 0x80, 0xED, 0xF5, 0xE0, 0xF4])
        fin = 0 if rng.random() < 0.05 else FIN
        pos = 0
        for f in range(i, j):
            b0 = (op | rsv1 if f == i else C_) | (fin if f == j - 1 else 0)
            frames.append((b0, bytes(body[pos:pos + int(lens[f])])))
            pos += int(lens[f])
        i = j
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tiny_many", "zero_len_runs", "packed_wire", "long_gaps"])
def test_layouts_masked_and_plain(kind):
    offs, lens, total = layout(kind, np.random.default_rng(5))
    frames = fill_messages(lens, 11)
    b = Batch(frames, offs, total)
    expect = check(b)  # plain and masked, each against the reference; the buffer unchanged (run_gpu)
    assert {ref.NOT_TEXT, ref.OK, ref.BAD} <= set(expect)


# ---------------------------------------------------------------- streams and carry

@functools.lru_cache(maxsize=None)
def stream_batch():
    rng = random.Random(37)
    streams = []
    for s in range(37):
        if s in (3, 4, 20, 36):
            streams.append([])
        elif s == 5:   # a cut inside a code point
            streams.append([(T_, b"x\xe2\x82"), (C_, b""), (C_ | FIN, b"\xacy")])
        elif s == 6:   # a cut between a BAD frame and its continuations
            streams.append([(T_, b"\xff"), (PING | FIN, b"\x80"), (C_, b"a"), (C_ | FIN, b"b"), (T_ | FIN, b"ok")])
        elif s == 7:   # a cut inside a binary message
            streams.append([(B_, b"\xff\xfe"), (C_, b"\xfd"), (C_ | FIN, b"\xfc")])
        elif s == 8:   # ends inside a code point at the cut, FIN on an empty frame after it
            streams.append([(T_, b"\xf0\x9f"), (C_ | FIN, b"")])
        else:
            streams.append(ref.random_stream(rng, rng.randint(1, 6), max_len=400))
    frames = [f for st in streams for f in st]
    first = np.concatenate([[0], np.cumsum([len(st) for st in streams])]).astype(np.int64)
    offs, total = packed_offsets([len(p) for _, p in frames], rng)
    expect = np.concatenate([np.array(ref.validate_stream(st)[0], dtype=np.uint8) for st in streams if st])
    return Batch(frames, offs, total), first, expect


@pytest.mark.gpu
def test_streams_in_one_call():
    b, first, expect = stream_batch()
    for m in (False, True):
        out, carry, st = run_gpu(b, masked=m, stream_first=first)
        assert st == 0
        assert np.array_equal(out, expect), np.nonzero(out != expect)[0][:10]
        assert {0, 1, 2, 3} <= set(out)


@pytest.mark.gpu
def test_streams_cut_into_two_calls_joined_by_the_carry():
    b, first, expect = stream_batch()
    rng = random.Random(38)
    s5, s6, s7, s8 = (int(first[s]) for s in (5, 6, 7, 8))
    cuts = {s5 + 1, s5 + 2, s6 + 1, s6 + 2, s6 + 3, s7 + 1, s7 + 2, s8 + 1, int(first[3]), int(first[21])}
    cuts |= {rng.randrange(1, b.n) for _ in range(10)}
    for c in sorted(cuts):
        f1 = np.minimum(first, c)
        f2 = np.maximum(first, c) - c
        out1, carry, st1 = run_gpu(b, stream_first=f1, lo=0, hi=c)
        out2, carry2, st2 = run_gpu(b, masked=True, stream_first=f2, carry_in=carry, lo=c)
        assert st1 == 0 and st2 == 0
        got = np.concatenate([out1, out2])
        assert np.array_equal(got, expect), (c, np.nonzero(got != expect)[0][:10])
        # streams that ended before the cut are empty in the second call: their carry passes through
        done = [s for s in range(37) if first[s + 1] <= c]
        assert np.array_equal(carry2[done], carry[done]), c


# ---------------------------------------------------------------- frame-scan shapes

def header_constant(header, name):
    """A constexpr integer of kuma_amd/csrc/<header>."""
    txt = open(os.path.join(ROOT, "kuma_amd", "csrc", header)).read()
    return int(re.search(r"constexpr \w+ %s = (\d+);" % name, txt).group(1))


# frames one block of the frame-state scan covers (FrameArraysWs: nblk = ceil(n / kBlock)), one a lane
SCAN_B = header_constant("kmws_common.hpp", "kBlock")
SCAN_R = header_constant("kmws_stream_scan.hpp", "kScanBlockFrames")  # aggregates one round of scan_aggregates takes
SCAN_U = SCAN_B * SCAN_R  # frames whose aggregates fill one round
SCAN_SHAPES = [1, 63, 64, 65, SCAN_B - 1, SCAN_B, SCAN_B + 1, 2 * SCAN_B + 1, SCAN_B * SCAN_B + 3]
SCAN_LAYOUTS = ["one_stream", "stream_per_frame", "block_edge_streams", "empty_streams"]
# carries (kmws_utf8_rule.hpp: flags, then the look-back, most recent byte first) and the reference's state for each
SCAN_CARRIES = {"pending": bytes([3, 0x82, 0xE2, 0, 0, 0, 0, 0]),  # a checked message that stopped inside U+20AC
                "bad": bytes([7, 0x61, 0, 0, 0, 0, 0, 0]),         # a checked message already reported BAD
                "binary": bytes([1, 0, 0, 0, 0, 0, 0, 0])}        # an open message that is not checked


def scan_carry_state(kind):
    st = ref.StreamState()
    if kind is not None:
        st.open, st.checked, st.bad = True, kind != "binary", kind == "bad"
        if kind == "pending":
            st.pending = ref.first_bad(b"\xe2\x82")[1]
    return st


def scan_stream_first(layout, n):
    if layout == "one_stream":
        return [0, n]
    if layout == "stream_per_frame":
        return list(range(n + 1))
    if layout == "block_edge_streams":  # every wave edge, so every block edge: a stream ends on a block's last lane
        return sorted({0, n} | set(range(64, n, 64)))
    a, b = n // 3, 2 * n // 3           # empty streams first, in the middle and last
    return [0, 0, 0, a, a, a, b, n, n, n]


def scan_carry_after(frames, verdicts, carry):
    """The carry a stream leaves (kmws_utf8_rule.hpp: utf8_carry_pack), from its
    frames, the reference's verdicts on them and the carry it came with."""
    is_open, checked, bad = bool(carry[0] & 1), bool(carry[0] & 2), bool(carry[0] & 4)
    tail = bytes([carry[3], carry[2], carry[1]])
    for (b0, p), v in zip(frames, verdicts):
        if (b0 & 0x0F) >= 8:
            continue
        if b0 & 0x0F:
            is_open, checked, bad, tail = True, (b0 & 0x0F) == 1 and not (b0 & RSV1), False, bytes(3)
        if is_open:
            tail = (tail + p)[-3:]
            bad |= v in (ref.BAD, ref.AFTER_BAD)
        if b0 & FIN:
            is_open = False
    if not is_open:
        return bytes(8)
    if not checked:
        return bytes([1, 0, 0, 0, 0, 0, 0, 0])
    return bytes([3 | (4 if bad else 0), tail[2], tail[1], tail[0], 0, 0, 0, 0])


@functools.lru_cache(maxsize=None)
def scan_case(layout, n):
    """-> (batch, stream_first, carry_in, expected verdicts, expected carry_out)."""
    first = scan_stream_first(layout, n)
    ns = len(first) - 1
    rng = random.Random(1000 * SCAN_LAYOUTS.index(layout) + n % 997)
    lens = [rng.randint(0, 3) for _ in range(n)]
    lens[0] = 1
    frames = fill_messages(lens, 50 + n % 997, streams=first)
    # the first stream's carry, also where that stream is empty; then every fifth stream a BAD or a binary carry
    owner0 = max(s for s in range(ns) if first[s] == 0)
    kinds = {s: ("bad" if s % 5 == 2 else "binary") for s in range(ns) if s % 5 in (2, 4) and first[s] < first[s + 1]}
    kinds.update({0: "pending", owner0: "pending"})
    frames[0] = (C_, b"\xac")  # completes the carried code point; the frames behind it continue that message
    for s, kind in kinds.items():
        if s != owner0 and first[s] < first[s + 1]:
            b0, p = frames[first[s]]
            frames[first[s]] = (C_ | (b0 & FIN), p)  # a CONTINUE of the carried message
    # the first stream of four frames or more ends in a message that is BAD, goes on and stays open
    long = [s for s in range(ns) if first[s + 1] - first[s] >= 4]
    if long:
        e = first[long[0] + 1]
        frames[e - 3:e] = [(T_, b"\xff"), (C_, b"a"), (C_, b"b")]
    carry_in = np.zeros((ns, 8), dtype=np.uint8)
    for s, kind in kinds.items():
        carry_in[s] = np.frombuffer(SCAN_CARRIES[kind], dtype=np.uint8)
    expect, carry_out = [], np.zeros((ns, 8), dtype=np.uint8)
    for s in range(ns):
        st_frames = frames[first[s]:first[s + 1]]
        res = ref.validate_stream(st_frames, scan_carry_state(kinds.get(s)))[0]
        expect += res
        carry_out[s] = np.frombuffer(scan_carry_after(st_frames, res, bytes(carry_in[s])), dtype=np.uint8)
    offs, total = packed_offsets([len(p) for _, p in frames], rng)
    return Batch(frames, offs, total, seed=n), first, carry_in, np.array(expect, dtype=np.uint8), carry_out


def test_scan_shapes_are_informative():
    """CPU, on the reference's verdicts: every case of 64 frames or more holds
    all four verdicts, the carried code point is completed by frame 0, and the
    streams leave every kind of carry."""
    left = set()
    for layout in SCAN_LAYOUTS:
        for n in SCAN_SHAPES:
            _, first, carry_in, expect, carry_out = scan_case(layout, n)
            assert len(expect) == n and expect[0] == ref.OK and carry_in[0].any(), (layout, n)
            assert n < 64 or {ref.OK, ref.BAD, ref.AFTER_BAD, ref.NOT_TEXT} <= set(expect), (layout, n, set(expect))
            left |= set(carry_out[:, 0])
    assert left == {0, 1, 3, 7}  # between messages, open unchecked, open checked, open checked and BAD


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_SHAPES)
@pytest.mark.parametrize("layout", SCAN_LAYOUTS)
def test_frame_scan_shapes(layout, n):
    """The frame-state scan over wave edges, block edges and more than one wave of
    aggregates (65,539 frames: 257 aggregates, still one round of the aggregate
    scan; test_frame_scan_rounds goes past it): 0-3 byte payloads, so code points
    straddle fragments and the state matters across every edge."""
    check_scan_case(layout, scan_case(layout, n))


def check_scan_case(layout, case):
    b, first, carry_in, expect, carry_want = case
    assert b.n < 64 or {ref.OK, ref.BAD, ref.AFTER_BAD, ref.NOT_TEXT} <= set(expect)
    one = layout == "one_stream"
    out, carry, st = run_gpu(b, masked=True, stream_first=None if one else first, carry_in=carry_in)
    assert st == 0
    bad = np.nonzero(out != expect)[0]
    assert bad.size == 0, (bad[:10], out[bad[:10]], expect[bad[:10]])
    bad = np.nonzero((carry != carry_want).any(axis=1))[0]
    assert bad.size == 0, (bad[:10], carry[bad[:10]], carry_want[bad[:10]])


# ---------------------------------------------------------------- frame-scan rounds

# Past one round of the aggregate scan (SCAN_R aggregates of SCAN_B frames): the round edge itself, round two in
# lanes 0 and 1, round two past a wave edge (an aggregate in lane 64: a lane takes four), round three.
ROUND_EDGE = [SCAN_U - 1, SCAN_U, SCAN_U + 1]
ROUND_TWO_LANE_1 = SCAN_U + 4 * SCAN_B + 1
ROUND_TWO_LANE_64 = SCAN_U + 256 * SCAN_B + 1
ROUND_THREE = 2 * SCAN_U + 3
SCAN_ROUND_CASES = [(layout, ROUND_TWO_LANE_1) for layout in SCAN_LAYOUTS] + \
    [(layout, n) for n in ROUND_EDGE + [ROUND_TWO_LANE_64, ROUND_THREE] for layout in ("one_stream", "block_edge_streams")]


def scan_aggregates_of(n):
    return -(-n // SCAN_B)


def test_scan_round_shapes_have_the_aggregates_they_claim():
    """CPU, from the header's constants."""
    assert scan_aggregates_of(max(SCAN_SHAPES)) == SCAN_B + 1 <= SCAN_R  # one round: more than one wave of aggregates
    assert [scan_aggregates_of(n) for n in ROUND_EDGE] == [SCAN_R, SCAN_R, SCAN_R + 1]
    assert scan_aggregates_of(ROUND_TWO_LANE_1) == SCAN_R + 5       # round two: four in lane 0, one in lane 1
    assert scan_aggregates_of(ROUND_TWO_LANE_64) == SCAN_R + 257    # round two: the last one in lane 256 / 4 = 64
    assert scan_aggregates_of(ROUND_TWO_LANE_64 - SCAN_B) == SCAN_R + 256  # and no smaller count has one there
    assert scan_aggregates_of(ROUND_THREE) == 2 * SCAN_R + 1 > 2 * SCAN_R
    assert ROUND_TWO_LANE_64 == 327681 and SCAN_U == 262144  # the figures as typed in the design


@pytest.mark.gpu
@pytest.mark.parametrize("layout,n", SCAN_ROUND_CASES)
def test_frame_scan_rounds(layout, n):
    """The second and third round of the aggregate scan: what round one composed
    (scan_aggregates' run) stands in front of every later aggregate."""
    check_scan_case(layout, scan_case.__wrapped__(layout, n))  # too large to keep


# ---------------------------------------------------------------- state across the round edge

def edge_fill():
    """Ordinary content to cut prefixes and tails from."""
    return fill_messages([k % 4 for k in range(2048)], 77)


def round_edge_frames(head_block, piece_block, second, tail=300):
    """One stream.  A text head without FIN whose payload ends in E2 in block
    head_block; `second` (82 completes the code point so far, 61 breaks it) in a
    CONTINUE in block piece_block, AC 21 in a CONTINUE|FIN in the block after it;
    between them only PINGs with payloads >= 0x80 and empty CONTINUEs, so what the
    head left has to travel through every block aggregate between.
    -> (frames, dict of the head's, the second piece's and the FIN's index)."""
    head, piece, fin = head_block * SCAN_B + 10, piece_block * SCAN_B + 20, (piece_block + 1) * SCAN_B + 30
    unit = edge_fill()
    frames = (unit * (head // len(unit) + 1))[:head]
    frames.append((T_, b"x\xe2"))
    pings = [(PING | FIN, bytes([0x80 + k, 0xBF - k])) for k in range(4)]
    frames += [pings[(i >> 1) & 3] if i & 1 else (C_, b"") for i in range(head + 1, fin)]
    frames[piece] = (C_, second)
    frames.append((C_ | FIN, b"\xac\x21"))
    frames += unit[:tail]
    return frames, dict(head=head, piece=piece, fin=fin)


OK_PIECE, BAD_PIECE = b"\x82", b"\x61"
# (head's block, second piece's block): around the edge of round one and of round two.  The pieces' aggregates
# lie in lane 1 of their round (a lane takes four), so the empty CONTINUEs of lane 0's four blocks and the pieces
# both need what the rounds before composed; "wave": in lane 64, past a wave edge of that round's block scan.
EDGE_ROUNDS = {2: (SCAN_R - 3, SCAN_R + 5), 3: (2 * SCAN_R - 3, 2 * SCAN_R + 5)}
EDGE_CASES = {"round2": EDGE_ROUNDS[2], "round2_wave": (SCAN_R - 3, SCAN_R + 257), "round3": EDGE_ROUNDS[3]}
# two calls: the head in the first, the cut inside the filler run, the pieces in lane 1 of the second call's round two
TWO_CALL_BLOCKS, TWO_CALL_CUT = (1, SCAN_R + 7), 2 * SCAN_B + 17


def round_edge_expect(frames, at, second):
    """The reference's verdicts, and the typed claims on them."""
    expect = want(frames)
    between = range(at["head"] + 1, at["fin"])
    empties = np.array([i for i in between if frames[i] == (C_, b"")])
    pings = np.array([i for i in between if frames[i][0] == PING | FIN])
    assert len(empties) + len(pings) + 1 == len(between) and (expect[pings] == ref.NOT_TEXT).all()
    assert expect[at["head"]] == ref.OK and (expect[empties[empties < at["piece"]]] == ref.OK).all()
    if second == OK_PIECE:
        assert (expect[empties] == ref.OK).all() and expect[at["piece"]] == ref.OK and expect[at["fin"]] == ref.OK
    else:
        assert expect[at["piece"]] == ref.BAD and expect[at["fin"]] == ref.AFTER_BAD
        assert (expect[empties[empties > at["piece"]]] == ref.AFTER_BAD).all()
    return expect


def round_edge_batch(frames, seed=3):
    rng = np.random.default_rng(seed)
    lens = np.array([len(p) for _, p in frames], dtype=np.int64)
    gaps = rng.integers(2, 15, size=len(frames))
    offs = np.cumsum(gaps + lens) - lens
    return Batch(frames, offs, int(offs[-1] + lens[-1]) + 5, seed=seed)


def test_round_edge_cases_straddle_the_rounds_they_claim():
    """CPU, from the header's constants: the head's block lies below the round
    edge and the FIN's above it with a whole filler block on either side, the
    pieces' aggregates in the lane the case names, in the second call of the
    two-call case too; and the reference's answers (round two)."""
    for name, (hb, pb) in EDGE_CASES.items():
        rnd = 3 if name == "round3" else 2
        edge = (rnd - 1) * SCAN_R  # the first aggregate of the round
        assert hb <= edge - 2 and edge + 1 <= pb  # blocks hb + 1 .. edge - 1 and edge .. pb - 1: whole, filler only
        assert (pb - edge) // 4 == (pb + 1 - edge) // 4 == (64 if name == "round2_wave" else 1)  # the pieces' lane
        if name == "round2":
            frames, at = round_edge_frames(hb, pb, OK_PIECE)
            assert at["head"] // SCAN_B == hb and at["piece"] // SCAN_B == pb and at["fin"] // SCAN_B == pb + 1
            assert scan_aggregates_of(len(frames)) > edge + 2
            for second in (OK_PIECE, BAD_PIECE):
                fr, _ = round_edge_frames(hb, pb, second)
                expect = round_edge_expect(fr, at, second)
                # cut off before the FIN, the stream stays inside the message
                left = scan_carry_after(fr[:at["fin"]], expect[:at["fin"]], bytes(8))
                assert left == (bytes([3, 0x82, 0xE2, 0x78, 0, 0, 0, 0]) if second == OK_PIECE else
                                bytes([7, 0x61, 0xE2, 0x78, 0, 0, 0, 0]))
    hb, pb = TWO_CALL_BLOCKS
    head, piece = hb * SCAN_B + 10, pb * SCAN_B + 20
    assert head < TWO_CALL_CUT < piece and (piece - TWO_CALL_CUT) // SCAN_B == SCAN_R + 5


@pytest.mark.gpu
@pytest.mark.parametrize("second", [OK_PIECE, BAD_PIECE], ids=["ok", "bad"])
@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_message_open_across_rounds(case, second):
    """The analogue of the msg and proto files' test_message_open_across_blocks:
    "open, checked, inside U+20AC" crosses the edge of round one (two) through
    scan_aggregates' run, not through any block's own scan.  Whole, and cut off
    before the FIN: the carry the stream leaves."""
    frames, at = round_edge_frames(*EDGE_CASES[case], second)
    expect = round_edge_expect(frames, at, second)
    b = round_edge_batch(frames)
    for hi in (b.n, at["fin"]):
        out, carry, st = run_gpu(b, masked=case == "round2", hi=hi)
        assert st == 0
        bad = np.nonzero(out != expect[:hi])[0]
        assert bad.size == 0, (hi, bad[:10], out[bad[:10]], expect[bad[:10]])
        left = scan_carry_after(frames[:hi], expect[:hi], bytes(8))
        assert bytes(carry[0]) == left, (hi, carry[0], left)
        if hi == at["fin"]:
            assert carry[0][0] == (3 if second == OK_PIECE else 7)


@pytest.mark.gpu
@pytest.mark.parametrize("second", [OK_PIECE, BAD_PIECE], ids=["ok", "bad"])
def test_message_open_across_rounds_in_two_calls(second):
    """The batch cut inside the filler run: in the second call the state comes in
    as carry_in at frame 0 and reaches the pieces in round two through run."""
    frames, at = round_edge_frames(*TWO_CALL_BLOCKS, second)
    expect = round_edge_expect(frames, at, second)
    b = round_edge_batch(frames)
    c = TWO_CALL_CUT
    out1, carry1, st1 = run_gpu(b, hi=c)
    assert st1 == 0 and bytes(carry1[0]) == bytes([3, 0xE2, 0x78, 0, 0, 0, 0, 0])
    out2, carry2, st2 = run_gpu(b, masked=True, carry_in=carry1, lo=c)
    assert st2 == 0
    got = np.concatenate([out1, out2])
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, (bad[:10], got[bad[:10]], expect[bad[:10]])
    assert bytes(carry2[0]) == scan_carry_after(frames, expect, bytes(8))


# ---------------------------------------------------------------- contract

@pytest.mark.gpu
def test_contract_bad_descriptors_streams_and_empty_batch():
    frames = [(T_ | FIN, b"abc"), (T_ | FIN, "€".encode()), (T_ | FIN, b"\xff"), (T_ | FIN, b"z" * 40)]
    good = Batch(frames, [4, 20, 40, 60], 128)
    out, _, st = run_gpu(good)
    assert st == 0 and list(out) == [1, 1, 2, 1]
    unsorted = Batch(frames, [4, 40, 20, 60], 128)
    unsorted.offs = np.array([4, 40, 20, 60])
    assert run_gpu(unsorted)[2] & 1
    overlap = Batch(frames, [4, 20, 40, 60], 128)
    overlap.offs = np.array([4, 5, 40, 60])
    assert run_gpu(overlap)[2] & 1
    past = Batch(frames, [4, 20, 40, 60], 128)
    past.offs = np.array([4, 20, 40, 100])
    assert run_gpu(past)[2] & 1
    for sf in ([0, 3, 2, 4], [1, 2, 4], [0, 2, 3], [0, 5, 4]):
        assert run_gpu(good, stream_first=sf)[2] & 1, sf
    assert run_gpu(good, stream_first=[0, 0, 2, 2, 4, 4])[2] == 0
    # n == 0: OK, carry_out = carry_in
    carry = np.arange(24, dtype=np.uint8).reshape(3, 8)
    out, co, _ = run_gpu(good, stream_first=[0, 0, 0, 0], carry_in=carry, lo=0, hi=0)
    assert out.size == 0 and np.array_equal(co, carry)
    out, co, _ = run_gpu(good, lo=0, hi=0)
    assert np.array_equal(co, np.zeros((1, 8), dtype=np.uint8))


@pytest.mark.gpu
def test_validate_in_a_captured_graph_follows_the_payload():
    import torch as T
    from kuma_amd import kmws
    data = ref.text(random.Random(9), 50000)
    frames = [(T_ | FIN, data), (T_ | FIN, b"tail")]
    b = Batch(frames, [6, 50020], 50040)
    keep = {}
    out0, _, st = run_gpu(b, keep=keep)  # warm: every kernel loaded before the capture
    assert st == 0 and list(out0) == [1, 1]
    base, descs, fl, out, ws = (keep[k] for k in ("base", "descs", "fl", "out", "ws"))
    s = T.cuda.Stream()
    s.wait_stream(T.cuda.current_stream())
    with T.cuda.stream(s):
        kmws.utf8_validate(base, descs, fl, out, ws, span=b.total)
    T.cuda.current_stream().wait_stream(s)
    T.cuda.synchronize()
    g = T.cuda.CUDAGraph()
    with T.cuda.graph(g):
        kmws.utf8_validate(base, descs, fl, out, ws, span=b.total)
    T.cuda.synchronize()
    p = 6 + 33333
    for newb, verdict in ((0xFF, 2), (b.plain[p], 1)):
        base[p] = int(newb)
        out.fill_(0xEE)
        g.replay()
        T.cuda.synchronize()
        assert ws.status() == 0
        assert list(out.cpu().numpy()[:2]) == [verdict, 1]


# ---------------------------------------------------------------- fuzz

FUZZ_BATCHES = 20


@functools.lru_cache(maxsize=None)
def fuzz_batch(k):
    rng = random.Random(9000 + k)
    pool = fuzz_pool()
    ns = rng.randint(3, 12)
    deck = ["ok", "bad", "bin", "ok", "bad", "rsv", "bad", "ok"]  # the mix is dealt, not drawn
    streams, m, late_done = [], rng.randrange(8), False
    for s in range(ns):
        st = []
        for _ in range(rng.randint(3, 8) if s < 3 else rng.randint(0, 8)):
            kind = deck[m % len(deck)]
            m += 1
            big = rng.random() < 0.12
            n = rng.randint(20000, 70000) if big else rng.choice([0, 1, 2, 3, 5, 16, 100, 700, 3000])
            if kind == "bad":
                n = max(n, 2)
            body = bytearray(pool.take(rng, n))
            parts = None
            if kind == "bad" and not late_done:  # the BAD frame after the first: the last byte, in a later fragment
                body[-1] = 0xFF
                cut = rng.randint(1, n - 1)
                parts, late_done = [bytes(body[:cut]), bytes(body[cut:])], True
            elif kind == "bad":
                body[rng.randrange(n)] = rng.choice([0xFF, 0xFF, 0xC0, 0xF5, 0xFE, 0xC1])
            if parts is None:
                parts = ref.fragment(rng, bytes(body), 6)
            op, rsv1 = (B_ if kind == "bin" else T_), kind == "rsv"
            for fr in ref.message(parts, op, rsv1, fin=rng.random() < 0.95):
                if rng.random() < 0.1:
                    st.append((rng.choice([9, 10]) | FIN, bytes(rng.randrange(0x80, 0x100) for _ in range(5))))
                st.append(fr)
        streams.append(st)
    frames = [f for st in streams for f in st]
    first = np.concatenate([[0], np.cumsum([len(st) for st in streams])]).astype(np.int64)
    offs, total = packed_offsets([len(p) for _, p in frames], rng)
    assert total <= 2 << 20
    per_stream = [ref.validate_stream(st)[0] for st in streams]
    expect = np.array([v for r in per_stream for v in r], dtype=np.uint8)
    return Batch(frames, offs, total, seed=k), first, expect, streams, per_stream


@functools.lru_cache(maxsize=None)
def fuzz_pool():
    return ref.TextPool(random.Random(8999))


def fuzz_mix(streams, per_stream):
    """(valid, invalid, invalid with the BAD frame after the first) checked messages."""
    valid = invalid = late = 0
    for st, res in zip(streams, per_stream):
        msgs, cur = [], None
        for (b0, _), v in zip(st, res):
            if (b0 & 0x0F) >= 8:
                continue
            if b0 & 0x0F:
                cur = []
                msgs.append(cur)
            if cur is not None:
                cur.append(v)
            if b0 & FIN:
                cur = None
        for m in msgs:
            if m[0] == ref.NOT_TEXT:
                continue
            if ref.BAD in m:
                invalid += 1
                late += m.index(ref.BAD) != 0
            else:
                valid += 1
    return valid, invalid, late


def test_fuzz_mix_is_informative():
    """CPU, on the reference's verdicts: per batch at least a quarter of the
    checked messages valid, a quarter invalid, and an invalid one whose BAD frame
    is not its first."""
    for k in range(FUZZ_BATCHES):
        _, _, _, streams, per_stream = fuzz_batch(k)
        valid, invalid, late = fuzz_mix(streams, per_stream)
        tot = valid + invalid
        assert tot >= 4 and valid * 4 >= tot and invalid * 4 >= tot and late >= 1, (k, valid, invalid, late)


@pytest.mark.gpu
def test_fuzz():
    for k in range(FUZZ_BATCHES):
        b, first, expect, streams, per_stream = fuzz_batch(k)
        valid, invalid, late = fuzz_mix(streams, per_stream)
        assert valid * 4 >= valid + invalid and invalid * 4 >= valid + invalid and late >= 1
        out, _, st = run_gpu(b, masked=bool(k & 1), stream_first=first)
        assert st == 0
        bad = np.nonzero(out != expect)[0]
        assert bad.size == 0, (k, bad[:10], out[bad[:10]], expect[bad[:10]])
