"""kmws_decoder_set_utf8_check on the GPU: the opt-in UTF-8 check of text
messages on the host path (kmws_decoder_feed, kmws_decoder_feed_deferred /
kmws_rx_batch_*), whose payload pass is unmask_pieces_utf8_kernel.

Reference: tests/utf8_ref.py (validate_stream on one connection's (header byte
0, plain payload) list), which tests/test_utf8_ref.py pins against bytes.decode.

Every case goes through three routes, so that staged (16-byte aligned) and
unaligned hulls both occur:
  (i)   pageable bytes into handleData (payloads staged at aligned offsets);
  (ii)  a pinned torch CPU tensor through handleDataPtr (payloads unmasked /
        checked in place, at header-length offsets 6 / 8 / 14);
  (iii) an RxBatch with an attached pinned ring, flush as well as submit + poll.
Every case asserts the verdicts equal the reference's, and that payload bytes
and return codes equal those of the same feed with the check off."""
import random

import numpy as np
import pytest
import torch

import utf8_ref as ref
from kuma_amd import kmws

gpu = pytest.mark.gpu

BUF_BYTES = 1 << 20
_bufs = {}


def pinned(name):
    """Two pinned buffers for the whole module: the read buffer of route (ii), the ring of route (iii)."""
    if name not in _bufs:
        _bufs[name] = torch.zeros(BUF_BYTES, dtype=torch.uint8).pin_memory()
    return _bufs[name]


def frame_wire(b0, payload, key):
    """One frame on the wire; key: 4 bytes (masked) or None."""
    n = len(payload)
    mask_bit = 0x80 if key is not None else 0
    if n < 126:
        hdr = bytes([b0, mask_bit | n])
    elif n < 65536:
        hdr = bytes([b0, mask_bit | 126]) + n.to_bytes(2, "big")
    else:
        hdr = bytes([b0, mask_bit | 127]) + n.to_bytes(8, "big")
    if key is None:
        return hdr + payload
    p = np.frombuffer(payload, dtype=np.uint8)
    k = np.frombuffer((key * (n // 4 + 1))[:n], dtype=np.uint8)
    return hdr + key + (p ^ k).tobytes()


def wire_of(frames, masked, seed=1):
    rng = random.Random(seed)
    return [frame_wire(b0, p, bytes(rng.randrange(256) for _ in range(4)) if masked else None) for b0, p in frames]


def chunks_of(wire, chunk):
    if not chunk:
        return [(0, len(wire))]
    return [(o, min(chunk, len(wire) - o)) for o in range(0, len(wire), chunk)]


def feed(route, wire, masked, check, cuts, handler=None, batch=None, base=0):
    """Feeds `wire` (bytes) cut at `cuts` [(offset, length)] through a route.
    -> (return codes, [(header byte 0, payload, utf8)], buffer bytes after the call or None)."""
    h = handler or kmws.WSHandler(kmws.SERVER if masked else kmws.CLIENT)
    if handler is None and check is not None:
        h.setUtf8Check(check)
    got = []

    def cb(hdr, payload):
        b0 = (hdr.fin << 7) | (hdr.rsv1 << 6) | (hdr.rsv2 << 5) | (hdr.rsv3 << 4) | hdr.opcode
        got.append((b0, payload, hdr.utf8))

    h.setFrameCallback(cb)
    rcs, after = [], None
    if route == "bytes":
        for o, n in cuts:
            rcs.append(h.handleData(wire[o:o + n]))
    elif route == "pinned":
        t = pinned("read")
        assert base + len(wire) <= BUF_BYTES
        t[base:base + len(wire)] = torch.frombuffer(bytearray(wire), dtype=torch.uint8)
        for o, n in cuts:
            rcs.append(h.handleDataPtr(t.data_ptr() + base + o, n))
        after = bytes(t[base:base + len(wire)].numpy().tobytes())
    else:  # "ring_flush", "ring_poll"
        b = batch or kmws.RxBatch()
        ring = pinned("ring")
        if batch is None:
            b.attach_ring(ring)
        assert base + len(wire) <= BUF_BYTES
        ring[base:base + len(wire)] = torch.frombuffer(bytearray(wire), dtype=torch.uint8)
        for o, n in cuts:
            rcs.append(h.handleDataDeferredPtr(b, ring.data_ptr() + base + o, n))
            if route == "ring_poll":
                b.submit()
        if route == "ring_poll":
            b.poll(wait=True)
        else:
            b.flush()
        assert b.pending() == 0 and b.inflight() == 0
    return rcs, got, after


ROUTES = ("bytes", "pinned", "ring_flush", "ring_poll")


def check_case(frames, masked=True, chunk=0, routes=ROUTES, seed=1, per_frame_cuts=False):
    """Runs one connection's frames through every route with the check on and
    off; asserts verdicts == reference, bytes and return codes == check off."""
    want, _ = ref.validate_stream(frames)
    parts = wire_of(frames, masked, seed)
    wire = b"".join(parts)
    if per_frame_cuts:  # one feed (and, on the ring, one submit) per frame
        cuts, o = [], 0
        for p in parts:
            cuts.append((o, len(p)))
            o += len(p)
    else:
        cuts = chunks_of(wire, chunk)
    for route in routes:
        rc_on, got_on, after_on = feed(route, wire, masked, True, cuts)
        rc_off, got_off, after_off = feed(route, wire, masked, False, cuts)
        assert [(b0, p) for b0, p, _ in got_on] == [(b0, p) for b0, p in frames], route
        assert [g[2] for g in got_on] == want, (route, [g[2] for g in got_on], want)
        assert [(b0, p) for b0, p, _ in got_off] == [(b0, p) for b0, p in frames], route
        assert all(g[2] == 0 for g in got_off), route
        assert rc_on == rc_off, route
        assert after_on == after_off, route
        if route == "pinned" and not masked:
            assert after_on == wire, "CLIENT mode: the pinned buffer is untouched"
    return want


# ---- 1. lengths ----

LENGTHS = [0, 1, 2, 3, 4, 15, 16, 17, 1023, 1024, 1025, 16383, 16384, 16385, 40000]


@gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_valid_and_cut_short(n):
    rng = random.Random(1000 + n)
    valid = ref.text(rng, n)
    assert check_case([(0x81, valid)]) == [ref.OK]
    if n:
        j = min(n, 3)
        cut = ref.text(rng, n - j) + "\U0001F600".encode()[:j]  # ends inside a 4-byte code point: rule (b)
        assert len(cut) == n
        assert check_case([(0x81, cut)]) == [ref.BAD]


# ---- 2. boundary straddles ----

CP4, CP3 = "\U0001F600".encode(), "€".encode()
# the boundary's distance from the hull's first word: a 16-byte word, a 1 KiB row, the 16 KiB pieces
BOUNDARIES = [48, 1024, 16384, 32768]
# a payload byte's position relative to the hull: route (i) stages payloads at aligned offsets (shift 0); routes
# (ii) / (iii) leave them behind their 8-byte header (126-class length + key) at the start of the pinned buffer
SHIFTS = [0, 8]


def straddle_payload(rng, pool, boundary, shift, cp, k, corrupt=None):
    """Text whose code point `cp` has its k-th internal cut on the boundary:
    the cut is at payload position boundary - shift."""
    bpos = boundary - shift
    start = bpos - k
    body = bytearray(pool.take(rng, start) + cp + pool.take(rng, 61))
    if corrupt == "before":
        body[bpos - 1] = 0x41
    elif corrupt == "after":
        body[bpos] = 0x41
    return bytes(body)


@gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_boundary_straddles(boundary):
    rng = random.Random(boundary)
    pool = ref.TextPool(rng, 1 << 16)
    for shift in SHIFTS:
        if shift and boundary == 48:
            continue  # a payload this short has a 6-byte header: test_word_boundary_unaligned
        routes = ("bytes",) if shift == 0 else ("pinned", "ring_flush")
        for cp in (CP4, CP3):
            for k in range(1, len(cp)):
                p = straddle_payload(rng, pool, boundary, shift, cp, k)
                assert shift == 0 or 126 <= len(p) < 65536  # the 8-byte header SHIFTS assumes
                assert check_case([(0x81, p)], routes=routes) == [ref.OK]
                for corrupt in ("before", "after"):
                    if corrupt == "before" and k == 1:
                        continue  # the byte before the cut is the lead
                    bad = straddle_payload(rng, pool, boundary, shift, cp, k, corrupt)
                    assert check_case([(0x81, bad)], routes=routes) == [ref.BAD]


@gpu
def test_word_boundary_unaligned():
    """Boundary 48 on routes (ii) / (iii): a short payload sits behind a 6-byte
    header, so the word boundary is at payload position 48 - 6."""
    rng = random.Random(6)
    pool = ref.TextPool(rng, 1 << 12)
    for cp in (CP4, CP3):
        for k in range(1, len(cp)):
            for corrupt in (None, "before", "after"):
                if corrupt == "before" and k == 1:
                    continue
                p = straddle_payload(rng, pool, 48, 6, cp, k, corrupt)
                assert len(p) < 126
                want = [ref.OK] if corrupt is None else [ref.BAD]
                assert check_case([(0x81, p)], routes=("pinned", "ring_flush")) == want


@gpu
@pytest.mark.parametrize("lead,second", [(0xE0, 0x80), (0xED, 0xA0), (0xF0, 0x80), (0xF4, 0x90)])
def test_narrowed_range_violation_across_the_piece_edge(lead, second):
    """The lead is the piece's last byte; the byte that breaks its narrowed
    range is the next piece's first -- judged from the host-supplied edge."""
    rng = random.Random(lead)
    pool = ref.TextPool(rng, 1 << 16)
    rest = b"\x80" * (2 if lead >= 0xF0 else 1)
    for shift, routes in ((0, ("bytes",)), (8, ("pinned", "ring_flush", "ring_poll"))):
        start = 16384 - shift - 1
        p = pool.take(rng, start) + bytes([lead, second]) + rest + pool.take(rng, 40)
        assert check_case([(0x81, p)], routes=routes) == [ref.BAD]
        ok_second = {0xE0: 0xA0, 0xED: 0x9F, 0xF0: 0x90, 0xF4: 0x8F}[lead]
        p = pool.take(rng, start) + bytes([lead, ok_second]) + rest + pool.take(rng, 40)
        assert check_case([(0x81, p)], routes=routes) == [ref.OK]


# ---- 3. fragments ----

def fragment_cases():
    body = b"ab" + CP4 + b"cd"
    cases = []
    for cut in range(2, 7):  # before, inside (3 positions) and after the code point
        cases.append([(0x01, body[:cut]), (0x00, b""), (0x89, b"\xff\xfe"), (0x80, body[cut:])])
    for cut in range(3, 6):  # an empty FIN while the code point is pending: BAD on that frame
        cases.append([(0x01, body[:cut]), (0x8A, b""), (0x00, b""), (0x80, b"")])
    # three fragments, both cuts inside the code point
    cases.append([(0x01, body[:3]), (0x00, body[3:4]), (0x89, b""), (0x00, body[4:5]), (0x80, body[5:])])
    return cases


@gpu
@pytest.mark.parametrize("i", range(len(fragment_cases())))
def test_fragments_cut_inside_a_code_point(i):
    frames = fragment_cases()[i]
    want = check_case(frames)
    if frames[-1][1] == b"" and frames[0][1][-1] >= 0x80:
        assert want[-1] == ref.BAD and want[0] == ref.OK


# ---- 4. feed boundaries ----

def fragmented_stream():
    rng = random.Random(44)
    pool = ref.TextPool(rng, 1 << 14)
    frames = []
    for n in (700, 2300, 5000):
        body = pool.take(rng, n)
        parts = ref.fragment(rng, body, max_parts=4)
        frames += ref.message(parts)
        frames.append((0x89, b"\x80\x81"))
    bad = bytearray(pool.take(rng, 1500))
    bad[700] = 0xFF
    frames += ref.message([bytes(bad[:300]), bytes(bad[300:900]), bytes(bad[900:])])
    return frames


@gpu
@pytest.mark.parametrize("chunk", [1, 7, 4096])
def test_feed_boundaries(chunk):
    """The same wire in chunks of 1, 7 and 4096 bytes: frames reassembled across
    feeds (kStagedMasked; kHeld in CLIENT mode) keep the message state."""
    frames = fragmented_stream()
    routes = ("bytes", "pinned", "ring_flush")
    want = check_case(frames, chunk=chunk, routes=routes)
    assert ref.BAD in want and ref.AFTER_BAD in want and ref.OK in want
    check_case(frames, masked=False, chunk=chunk, routes=routes)


@gpu
def test_one_fragment_per_submit_single_poll():
    """Every frame its own generation, all in flight, one poll(wait) at the
    end: the state crosses generations in flight."""
    frames = fragmented_stream()
    check_case(frames, routes=("ring_poll",), per_frame_cuts=True)
    check_case(frames, masked=False, routes=("ring_poll",), per_frame_cuts=True)


@gpu
@pytest.mark.parametrize("base", [5, 13, 16])
def test_pinned_chunk_at_an_unaligned_address(base):
    """The caller's pinned chunk does not start on a 16-byte boundary: its
    descriptors are rebased onto the aligned base below it, and so are the
    edge words the host reads (a 40,000-byte frame: three pieces)."""
    rng = random.Random(base)
    pool = ref.TextPool(rng, 1 << 16)
    big = bytearray(pool.take(rng, 40000))
    frames = fragmented_stream() + [(0x81, bytes(big))]
    big[16384 - base - 8 + 1] = 0xFF  # near the first piece edge of the in-place hull
    frames += [(0x81, bytes(big))]
    want, _ = ref.validate_stream(frames)
    wire = b"".join(wire_of(frames, True))
    cuts = chunks_of(wire, 0)
    for route in ("pinned", "ring_flush"):
        rc_on, got_on, after_on = feed(route, wire, True, True, cuts, base=base)
        rc_off, got_off, after_off = feed(route, wire, True, False, cuts, base=base)
        assert [g[2] for g in got_on] == want and want[-2:] == [ref.OK, ref.BAD]
        assert [(b0, p) for b0, p, _ in got_on] == frames == [(b0, p) for b0, p, _ in got_off]
        assert rc_on == rc_off and after_on == after_off


# ---- 5. message sequence ----

@gpu
def test_message_sequence():
    ff = b"\xff" * 40
    frames = [(0x01, b"abc\xff"), (0x00, b"def"), (0x80, b"ghi"),          # BAD, AFTER_BAD, AFTER_BAD
              (0x01, "grü".encode()), (0x80, "ße".encode()),      # OK, OK
              (0x02, ff), (0x80, ff),                                        # binary: 0, 0
              (0x41, ff), (0x00, ff), (0x80, ff),                            # RSV1 text: 0, 0, 0
              (0x80, ff)]                                                    # CONTINUE with no open message: 0
    want = check_case(frames)
    assert want == [2, 3, 3, 1, 1, 0, 0, 0, 0, 0, 0]


# ---- 6. CLIENT mode: unmasked frames, the key-0 check-only job ----

@gpu
def test_client_mode_check_only():
    rng = random.Random(66)
    pool = ref.TextPool(rng, 1 << 16)
    bad = bytearray(pool.take(rng, 20000))
    bad[16390] = 0xC0
    frames = [(0x81, pool.take(rng, 300)), (0x01, pool.take(rng, 17000)), (0x80, pool.take(rng, 5)),
              (0x82, bytes(rng.randrange(256) for _ in range(500))), (0x81, bytes(bad)), (0x81, b""),
              (0x01, b"x\xe2\x82"), (0x80, b"")]
    want = check_case(frames, masked=False)
    assert want == [1, 1, 1, 0, 2, 1, 1, 2]


# ---- 7 / 8. three decoders interleaved into one RxBatch ----

SEED7 = 7


def three_streams():
    rng = random.Random(SEED7)
    streams = [ref.random_stream(rng, 12, max_len=3000) for _ in range(3)]
    return streams


def test_seed_covers_every_verdict():
    """Picked on the CPU: the reference itself produces all four values (and
    about 200 frames), so the interleaved test cannot pass vacuously."""
    streams = three_streams()
    seen = set()
    for s in streams:
        seen |= set(ref.validate_stream(s)[0])
    assert seen == {ref.NOT_TEXT, ref.OK, ref.BAD, ref.AFTER_BAD}
    assert 100 <= sum(len(s) for s in streams) <= 300


@gpu
@pytest.mark.parametrize("check", [True, False], ids=["check_on", "check_off"])
def test_three_decoders_interleaved_in_one_batch(check):
    streams = three_streams()
    wants = [ref.validate_stream(s)[0] for s in streams]
    wires = [wire_of(s, True, seed=70 + i) for i, s in enumerate(streams)]
    ring = pinned("ring")
    batch = kmws.RxBatch()
    batch.attach_ring(ring)
    handlers, gots = [], [[] for _ in streams]
    for i in range(3):
        h = kmws.WSHandler(kmws.SERVER)
        h.setUtf8Check(check)

        def cb(hdr, payload, i=i):
            b0 = (hdr.fin << 7) | (hdr.rsv1 << 6) | (hdr.rsv2 << 5) | (hdr.rsv3 << 4) | hdr.opcode
            gots[i].append((b0, payload, hdr.utf8))

        h.setFrameCallback(cb)
        handlers.append(h)
    # round robin, a few frames per read, alternately in the ring (in place) and
    # as bytes (staged); a submit every third round, polled while feeding
    rng = random.Random(SEED7 + 1)
    pos, ring_off, rnd = [0, 0, 0], 0, 0
    while any(pos[i] < len(wires[i]) for i in range(3)):
        for i in range(3):
            take = rng.randint(1, 4)
            part = b"".join(wires[i][pos[i]:pos[i] + take])
            pos[i] += take
            if not part:
                continue
            if rng.random() < 0.5:
                assert ring_off + len(part) <= BUF_BYTES
                ring[ring_off:ring_off + len(part)] = torch.frombuffer(bytearray(part), dtype=torch.uint8)
                rc = handlers[i].handleDataDeferredPtr(batch, ring.data_ptr() + ring_off, len(part))
                ring_off += len(part)
            else:
                rc = handlers[i].handleDataDeferred(batch, part)
            assert rc == kmws.WS_NOERR
        rnd += 1
        if rnd % 3 == 0:
            batch.submit()
            batch.poll()
    batch.flush()
    for i in range(3):
        assert [(b0, p) for b0, p, _ in gots[i]] == streams[i]
        assert [g[2] for g in gots[i]] == (wants[i] if check else [0] * len(streams[i]))
