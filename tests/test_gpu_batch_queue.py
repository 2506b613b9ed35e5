"""The host path under kmws_rx_batch_* / kmws_tx_batch_* and the synchronous
feed: the generation queue both batches keep (stages taken, rotated, retired
and reused; the attached ring) and the one launch body of the pinned stage
(kuma_amd/csrc/kmws_decoder.cpp, kmws_host_util.hpp).

References: delivered payloads and buffers unmasked in place equal the oracle's
decode of the same wire (oracle.Decoder), masked sends equal the oracle's
sendWsFrame (test_gpu_tx.oracle_send), verdicts equal tests/utf8_ref.py
validate_stream.  Wire, routes and straddling text are those of
tests/test_gpu_decoder_utf8.py.

The path matrix runs every source of descriptors -- staged, in another pinned
buffer, both in one job -- through every way a job can go:
  resident  3 frames of 100-4000 bytes: fits the resident worker;
  count     KMWS_RESIDENT_MAX_PAYLOADS + 1 frames of 1-64 bytes: launches;
  size      a frame of 2 x 16 KiB + 1 bytes at an address = 5 mod 16 (where the
            source can place it) beside a 1-byte frame: three pieces, so piece
            records j >= 1, the rebased offsets and the host-read edge words
            are in play; with the check on also with an ill-formed sequence and
            with a well-formed 4-byte code point astride the first piece edge.
Every shape runs with the thread's resident worker on and off
(kmws_resident_enable): 32 KiB + 2 bytes are below KMWS_RESIDENT_MAX_BYTES and
KMWS_RESIDENT_MAX_CHECKED_BYTES, so with the worker on the size shape is posted,
and with it off every shape launches -- asserted through the worker's job count
where the way is certain (worker off; the count shape)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import test_gpu_decoder_utf8 as du
import utf8_ref as ref
from kuma_amd import kmws
from oracle import oracle as orc
from test_gpu_tx import oracle_send

pytestmark = pytest.mark.gpu

MAX_PAYLOADS = 128  # KMWS_RESIDENT_MAX_PAYLOADS
PIECE = 16384       # a piece of the launched kernel: 16 KiB from the payload's aligned hull start
WARM_STAGES = 4     # kWarmStages: stages a batch makes at create
INPLACE_SHIFT = 5   # address of an in-place payload, mod 16


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")


def L():
    return kmws.lib()


def b0_of(hdr):
    return (hdr.fin << 7) | (hdr.rsv1 << 6) | (hdr.rsv2 << 5) | (hdr.rsv3 << 4) | hdr.opcode


def collector(got, tag=None):
    def cb(hdr, payload):
        got.append((b0_of(hdr), payload, hdr.utf8) if tag is None else (tag, b0_of(hdr), payload, hdr.utf8))
    return cb


def oracle_decode(parts, mode):
    """The oracle's decode of the wire parts, each in place: ([(byte 0, payload)], [part after the call])."""
    d = orc.Decoder(mode)
    after = []
    for p in parts:
        buf = bytearray(p)
        assert d.feed(buf) == 0
        after.append(bytes(buf))
    return [((f.fin << 7) | (f.rsv1 << 6) | (f.rsv2 << 5) | (f.rsv3 << 4) | f.opcode, f.payload) for f in d.frames], after


def ring_write(ring, off, data):
    ring[off:off + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8)


def ring_read(ring, off, n):
    return ring[off:off + n].numpy().tobytes()


def place(pos, lead):
    """The first offset >= pos at which a payload `lead` bytes further on lies at INPLACE_SHIFT mod 16."""
    return pos + (INPLACE_SHIFT - lead - pos) % 16


class worker:
    """The calling thread's resident worker on or off for the scope."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if not self.on:
            kmws.resident_enable(False)
        self.jobs = kmws.resident_info()["jobs"]
        return self

    def posted(self):
        return kmws.resident_info()["jobs"] - self.jobs

    def __exit__(self, *exc):
        if not self.on:
            kmws.resident_enable(True)


# ---- 1. attach rules ----

def pageable_ptr(keep, n=4096):
    buf = (C.c_uint8 * n)()
    keep.append(buf)
    return C.addressof(buf)


def test_rx_attach_rules():
    keep = []
    b = kmws.RxBatch()
    ring = du.pinned("ring")
    attach = L().kmws_rx_batch_attach_ring
    assert attach(b._b, pageable_ptr(keep), 4096) == kmws.ERR_INVALID_PARAM
    assert attach(b._b, ring.data_ptr(), 0) == kmws.ERR_INVALID_PARAM
    assert attach(b._b, ring.data_ptr(), ring.numel()) == kmws.OK
    assert attach(b._b, None, 0) == kmws.OK  # detach
    assert attach(b._b, ring.data_ptr(), ring.numel()) == kmws.OK
    h = kmws.WSHandler(kmws.SERVER)
    got = []
    h.setFrameCallback(collector(got))
    wire = du.frame_wire(0x82, b"pending", b"\x01\x02\x03\x04")
    assert h.handleDataDeferred(b, wire) == kmws.WS_NOERR and b.pending() == 1
    assert attach(b._b, ring.data_ptr(), ring.numel()) == kmws.ERR_INVALID_STATE  # a frame pending
    assert attach(b._b, None, 0) == kmws.ERR_INVALID_STATE
    assert b.submit() == 1 and b.pending() == 0 and b.inflight() == 1
    assert attach(b._b, ring.data_ptr(), ring.numel()) == kmws.ERR_INVALID_STATE  # a generation in flight
    assert b.flush() == 1 and b.inflight() == 0
    assert attach(b._b, ring.data_ptr(), ring.numel()) == kmws.OK  # again after a flush
    assert attach(b._b, None, 0) == kmws.OK
    # detached: a read that lies in the former ring is staged, the ring keeps its masked bytes
    ring_write(ring, 64, wire)
    assert h.handleDataDeferredPtr(b, ring.data_ptr() + 64, len(wire)) == kmws.WS_NOERR
    assert b.flush() == 1
    assert got == [(0x82, b"pending", 0)] * 2 and ring_read(ring, 64, len(wire)) == wire


def test_tx_attach_rules():
    keep = []
    b = kmws.TxBatch()
    ring = du.pinned("ring")
    attach = L().kmws_tx_batch_attach_ring
    assert attach(b._b, pageable_ptr(keep), 4096) == kmws.ERR_INVALID_PARAM
    assert attach(b._b, ring.data_ptr(), 0) == kmws.ERR_INVALID_PARAM
    assert attach(b._b, ring.data_ptr(), ring.numel()) == kmws.OK
    assert attach(b._b, None, 0) == kmws.OK  # detach
    assert attach(b._b, ring.data_ptr(), ring.numel()) == kmws.OK
    hdr = kmws.Header(fin=1, opcode=2, mask=1, maskey=b"\x11\x22\x33\x44")
    seg = bytearray(b"pending")
    want = oracle_send(hdr, [seg])
    assert b.add(hdr, [seg]) == want[0] and b.pending() == 1
    assert attach(b._b, ring.data_ptr(), ring.numel()) == kmws.ERR_INVALID_STATE  # a frame pending
    assert attach(b._b, None, 0) == kmws.ERR_INVALID_STATE
    t = b.submit()
    assert t == 1 and b.pending() == 0
    assert attach(b._b, ring.data_ptr(), ring.numel()) == kmws.ERR_INVALID_STATE  # a generation in flight
    assert b.flush() == 0  # completes what is in flight
    assert bytes(seg) == want[1][0]
    assert attach(b._b, ring.data_ptr(), ring.numel()) == kmws.OK  # again after a flush
    assert attach(b._b, None, 0) == kmws.OK


def test_empty_submit_and_flush():
    rx, tx = kmws.RxBatch(), kmws.TxBatch()
    for _ in range(2):
        assert rx.submit() == 0 and rx.poll() == 0 and rx.poll(wait=True) == 0 and rx.flush() == 0
        assert rx.inflight() == 0 and rx.pending() == 0
        assert tx.submit() == 0 and tx.flush() == 0 and tx.pending() == 0
        assert tx.poll(0) is True and tx.poll(7, wait=True) is True  # nothing in flight: every ticket is done
    # an unmasked send queues nothing
    tx.add(kmws.Header(fin=1, opcode=2, mask=0), [bytearray(b"plain")])
    assert tx.pending() == 0 and tx.submit() == 0


# ---- 2. the entries a delivery callback may not call ----

@pytest.mark.parametrize("outer", ["poll", "flush"])
def test_rx_entries_refused_inside_a_delivery(outer):
    b = kmws.RxBatch()
    ring = du.pinned("ring")
    h, h2 = kmws.WSHandler(kmws.SERVER), kmws.WSHandler(kmws.SERVER)
    h2.setFrameCallback(lambda hd, p: None)
    frames = [(0x82, bytes([i]) * (50 + i)) for i in range(3)]
    wire = b"".join(du.wire_of(frames, True))
    got, inner = [], []

    def cb(hdr, payload):
        got.append((b0_of(hdr), payload))
        inner.append((h2.handleDataDeferred(b, wire), L().kmws_rx_batch_submit(b._b), L().kmws_rx_batch_poll(b._b, 0),
                      L().kmws_rx_batch_poll(b._b, 1), L().kmws_rx_batch_flush(b._b),
                      L().kmws_rx_batch_attach_ring(b._b, ring.data_ptr(), ring.numel()),
                      L().kmws_rx_batch_attach_ring(b._b, None, 0)))

    h.setFrameCallback(cb)
    assert h.handleDataDeferred(b, wire) == kmws.WS_NOERR and b.pending() == 3
    if outer == "poll":
        assert b.submit() == 3
        assert b.poll(wait=True) == 3
    else:
        assert b.flush() == 3
    assert got == frames
    assert inner == [(kmws.ERR_INVALID_STATE,) * 7] * 3
    assert b.pending() == 0 and b.inflight() == 0
    # and the batch works on afterwards
    assert h.handleDataDeferred(b, wire) == kmws.WS_NOERR and b.flush() == 3 and got == frames * 2


# ---- 3. more generations in flight than warm stages ----

GENS = 6
assert GENS > WARM_STAGES


def rx_generation_frames(seed):
    """Per generation (handler, in the ring, payload): staged / ring alternate,
    masked (SERVER handler 0) / unmasked (CLIENT handler 1) in pairs, every
    third text ill-formed."""
    rng = random.Random(seed)
    gens = []
    for i in range(GENS):
        p = bytearray(ref.text(rng, rng.randrange(200, 3000)))
        if i % 3 == 0:
            p[len(p) // 2] = 0xFF
        gens.append(((i // 2) % 2, i % 2 == 1, bytes(p)))
    return gens


@pytest.mark.parametrize("check", [False, True], ids=["check_off", "check_on"])
def test_rx_more_generations_in_flight_than_warm_stages(check):
    b = kmws.RxBatch()
    ring = du.pinned("ring")
    b.attach_ring(ring)
    hs = [kmws.WSHandler(kmws.SERVER), kmws.WSHandler(kmws.CLIENT)]
    got = []
    for i, h in enumerate(hs):
        h.setUtf8Check(check)
        h.setFrameCallback(collector(got, tag=i))
    pos = 0
    for rnd in range(2):  # the second round goes through the stages the first one retired
        gens = rx_generation_frames(60 + rnd)
        want, spans = [], []
        for hid, in_ring, p in gens:
            wire = du.frame_wire(0x81, p, bytes([7 + rnd, 1, 2, 3]) if hid == 0 else None)
            (b0, plain), = oracle_decode([wire], kmws.SERVER if hid == 0 else kmws.CLIENT)[0]
            verdict = ref.validate_stream([(0x81, p)])[0][0] if check else 0
            want.append((hid, b0, plain, verdict))
            if in_ring:
                pos = place(pos, len(wire) - len(p))
                ring_write(ring, pos, wire)
                assert hs[hid].handleDataDeferredPtr(b, ring.data_ptr() + pos, len(wire)) == kmws.WS_NOERR
                pos += len(wire)
            else:
                assert hs[hid].handleDataDeferred(b, wire) == kmws.WS_NOERR
            assert b.submit() == 1
        assert b.inflight() == GENS and b.pending() == 0 and got == []
        assert b.poll(wait=True) == GENS  # all six, in submit order
        assert got == want
        assert {w[3] for w in want} == ({ref.OK, ref.BAD} if check else {0})
        assert b.inflight() == 0
        got.clear()


def test_tx_more_generations_in_flight_than_warm_stages():
    b = kmws.TxBatch()
    ring = du.pinned("ring")
    b.attach_ring(ring)
    rng = random.Random(77)
    last = 0
    for rnd in range(2):
        pos, gens, tickets = 0, [], []
        for i in range(GENS):
            hdr = kmws.Header(fin=1, opcode=2, mask=1, maskey=bytes(rng.randrange(256) for _ in range(4)))
            page = bytearray(rng.randrange(256) for _ in range(rng.randrange(100, 2000)))
            plain = [bytes(page)]
            if i % 2:  # a segment in the ring in front of the pageable one: the key phase runs across both
                n = rng.randrange(100, 2000)
                pos = place(pos, 0)
                ring_write(ring, pos, bytes(rng.randrange(256) for _ in range(n)))
                plain.insert(0, ring_read(ring, pos, n))
                keepbuf = (C.c_uint8 * len(page)).from_buffer(page)
                wire_hdr = b.add_ptrs(hdr, [ring.data_ptr() + pos, C.addressof(keepbuf)], [n, len(page)])
                gens.append((page, plain, (pos, n), keepbuf))
                pos += n
            else:
                wire_hdr = b.add(hdr, [page])
                gens.append((page, plain, None, None))
            want_hdr, want_segs = oracle_send(hdr, plain)
            assert wire_hdr == want_hdr
            gens[-1] += (want_segs,)
            tickets.append(b.submit())
        assert tickets == list(range(last + 1, last + GENS + 1))
        last = tickets[-1]
        assert b.poll(tickets[2], wait=True) is True
        for k, (page, plain, where, _, want_segs) in enumerate(gens):
            # copied back for generations 1-3 and for those alone: 4-6 still hold their plain bytes
            assert bytes(page) == (want_segs[-1] if k < 3 else plain[-1]), k
        assert b.poll(tickets[5], wait=True) is True
        for page, plain, where, _, want_segs in gens:
            assert bytes(page) == want_segs[-1]
            if where:
                assert ring_read(ring, *where) == want_segs[0]
        assert b.poll(last + 1, wait=False) is True and b.poll(last + 100, wait=True) is True  # nothing in flight
        assert b.flush() == 0


# ---- 4. the path matrix ----

_shapes = {}


def shape_frames(shape, shift):
    """One connection's FIN text / binary frames of a shape; shift: the large
    payload's address mod 16 (the piece edge is at payload position PIECE - shift)."""
    if (shape, shift) in _shapes:
        return _shapes[(shape, shift)]
    rng = random.Random(f"{shape}/{shift}")
    if shape == "resident":
        bad = bytearray(ref.text(rng, rng.randrange(100, 4000)))
        bad[len(bad) // 3] = 0xFF
        frames = [(0x81, ref.text(rng, rng.randrange(100, 4000))), (0x81, bytes(bad)),
                  (0x82, bytes(rng.randrange(256) for _ in range(rng.randrange(100, 4000))))]
    elif shape == "count":
        frames = []
        for i in range(MAX_PAYLOADS + 1):
            p = bytearray(ref.text(rng, rng.randrange(1, 65)))
            if i % 7 == 3:
                p[0] = 0xFF
            frames.append((0x81, bytes(p)))
    else:
        pool = ref.TextPool(rng, 1 << 16)
        if shape == "size":
            big = pool.take(rng, 2 * PIECE + 1)
        else:  # a 4-byte code point whose second cut is on the piece edge; "size_bad": its third byte replaced
            big = du.straddle_payload(rng, pool, PIECE, shift, du.CP4, 2, "after" if shape == "size_bad" else None)
            big += pool.take(rng, 2 * PIECE + 1 - len(big))
        assert len(big) == 2 * PIECE + 1
        frames = [(0x81, big), (0x81, b"a")]
    _shapes[(shape, shift)] = frames
    return frames


RX_SOURCES = ["sync_pinned", "sync_pageable", "deferred_staged", "deferred_ring", "deferred_mixed",
              "deferred_mixed_swapped"]
RX_CASES = [(s, c) for s in ("resident", "count", "size") for c in (False, True)] + [("size_bad", True),
                                                                                     ("size_cp4", True)]


def rx_deferred(parts, frames, in_ring, check, how):
    """One generation: parts[i] through the attached ring (in place) where
    in_ring[i], else as bytes (staged).  -> (frames delivered, ring parts after)."""
    b = kmws.RxBatch()
    ring = du.pinned("ring")
    if any(in_ring):
        b.attach_ring(ring)
    h = kmws.WSHandler(kmws.SERVER)
    h.setUtf8Check(check)
    got, spans, pos = [], [], 0
    h.setFrameCallback(collector(got))
    for part, (_, payload), r in zip(parts, frames, in_ring):
        if r:
            pos = place(pos, len(part) - len(payload))
            ring_write(ring, pos, part)
            assert h.handleDataDeferredPtr(b, ring.data_ptr() + pos, len(part)) == kmws.WS_NOERR
            spans.append((pos, len(part)))
            pos += len(part)
        else:
            assert h.handleDataDeferred(b, part) == kmws.WS_NOERR
            spans.append(None)
    assert b.pending() == len(parts)
    if how == "flush":
        assert b.flush() == len(parts)
    else:
        assert b.submit() == len(parts) and b.inflight() == 1
        assert b.poll(wait=True) == len(parts)
    assert b.pending() == 0 and b.inflight() == 0
    return got, [ring_read(ring, *s) if s else None for s in spans]


@pytest.mark.parametrize("resident", [True, False], ids=["worker_on", "worker_off"])
@pytest.mark.parametrize("shape,check", RX_CASES, ids=[f"{s}-{'check' if c else 'plain'}" for s, c in RX_CASES])
@pytest.mark.parametrize("source", RX_SOURCES)
def test_rx_path_matrix(source, shape, check, resident):
    n_frames = len(shape_frames(shape, 0))
    if source in ("sync_pageable", "deferred_staged"):
        in_ring = [False] * n_frames
    elif source in ("sync_pinned", "deferred_ring"):
        in_ring = [True] * n_frames
    else:
        in_ring = [(i % 2 == 0) != source.endswith("swapped") for i in range(n_frames)]
    frames = shape_frames(shape, INPLACE_SHIFT if in_ring[0] else 0)  # the large frame is the first
    parts = du.wire_of(frames, True, seed=3)
    want_frames, want_after = oracle_decode(parts, kmws.SERVER)
    assert want_frames == frames
    want_utf8 = ref.validate_stream(frames)[0] if check else [0] * n_frames
    if shape == "size_bad":
        assert want_utf8 == [ref.BAD, ref.OK]
    elif check and shape.startswith("size"):
        assert want_utf8 == [ref.OK, ref.OK]
    with worker(resident) as w:
        if source.startswith("sync"):
            wire = b"".join(parts)
            lead = len(parts[0]) - len(frames[0][1])
            rcs, got, after = du.feed("pinned" if in_ring[0] else "bytes", wire, True, check, [(0, len(wire))],
                                      base=place(0, lead))
            assert rcs == [kmws.WS_NOERR]
            assert after is None or after == b"".join(want_after)
            runs = [got]
        else:
            runs = []
            for how in ("flush", "poll"):
                got, after = rx_deferred(parts, frames, in_ring, check, how)
                assert after == [a if r else None for a, r in zip(want_after, in_ring)], how
                runs.append(got)
        if not resident or shape == "count":
            assert w.posted() == 0  # launched
    for got in runs:
        assert [(b0, p) for b0, p, _ in got] == frames
        assert [u for _, _, u in got] == want_utf8


TX_SOURCES = ["tx_staged", "tx_ring", "tx_mixed", "tx_mixed_swapped"]


@pytest.mark.parametrize("resident", [True, False], ids=["worker_on", "worker_off"])
@pytest.mark.parametrize("shape", ["resident", "count", "size"])
@pytest.mark.parametrize("source", TX_SOURCES)
def test_tx_path_matrix(source, shape, resident):
    payloads = [p for _, p in shape_frames(shape, 0)]
    if source == "tx_staged":
        in_ring = [False] * len(payloads)
    elif source == "tx_ring":
        in_ring = [True] * len(payloads)
    else:
        in_ring = [(i % 2 == 0) != source.endswith("swapped") for i in range(len(payloads))]
    ring = du.pinned("ring")
    rng = random.Random(5)
    with worker(resident) as w:
        for how in ("flush", "poll"):
            b = kmws.TxBatch()
            if any(in_ring):
                b.attach_ring(ring)
            ring[:1 << 17] = 0xA5
            image = np.full(1 << 17, 0xA5, dtype=np.uint8)
            pos, pages = 0, []
            for p, r in zip(payloads, in_ring):
                hdr = kmws.Header(fin=1, opcode=1, mask=1, maskey=bytes(rng.randrange(256) for _ in range(4)))
                want_hdr, (want_seg,) = oracle_send(hdr, [p])
                if r:
                    pos = place(pos, 0)
                    ring_write(ring, pos, p)
                    image[pos:pos + len(p)] = np.frombuffer(want_seg, dtype=np.uint8)
                    assert b.add_ptrs(hdr, [ring.data_ptr() + pos], [len(p)]) == want_hdr
                    pos += len(p) + 3
                else:
                    page = bytearray(p)
                    assert b.add(hdr, [page]) == want_hdr
                    pages.append((page, want_seg))
            assert pos < (1 << 17) and b.pending() == len(payloads)
            if how == "flush":
                assert b.flush() == len(payloads)
            else:
                t = b.submit()
                assert t == 1 and b.pending() == 0
                assert b.poll(t, wait=True) is True
            assert np.array_equal(ring[:1 << 17].numpy(), image), how  # ring segments masked, nothing around them
            for page, want_seg in pages:
                assert bytes(page) == want_seg, how
        if not resident or shape == "count":
            assert w.posted() == 0  # launched
