"""CPU checks of tests/header_cases.py: the corpus really holds every record
kind at every byte phase and provokes every WSError, the oracle-based per-frame
model agrees with the golden decode vectors, the tail-sweep records are what
their names say, and the host header-chain walk (kmws_find_headers) equals the
oracle-based walk model on every stream of the list.  The device runs are in
tests/test_gpu_headers.py."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import header_cases as hc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [pytest.param(hc.SERVER, id="server"), pytest.param(hc.CLIENT, id="client")]


def test_the_issue_s_record_kinds_are_all_there():
    kinds = hc.record_kinds()
    assert len(kinds) == len(set(kinds))
    flag = [k for k in kinds if k[0] == "flag"]
    assert {(k[1], k[2]) for k in flag} == {(b0, m) for b0 in range(256) for m in (0, 1)}
    assert {k[3] for k in flag} == {hc.p7(0), hc.p7(5), hc.p7(125), hc.x16(126), hc.x64(65536)}
    assert len(flag) == 256 * 2 * 5
    length = [k for k in kinds if k[0] == "length"]
    forms = {k[3] for k in length}
    want = {hc.p7(0), hc.p7(1), hc.p7(125)} | {hc.x16(v) for v in (0, 125, 126, 127, 65535)}
    want |= {hc.x64(v) for v in (0, 125, 65535, 65536, hc.MAX_LEN, hc.MAX_LEN + 1)}
    want |= {hc.x64(p) for p in hc.quirk127_patterns()}  # the cap and cap + 1 are among them
    want |= {hc.x64("8000000000000000"), hc.x64("0000000080000000")}
    want |= {hc.x64(1 << (8 * k)) for k in range(8)}
    assert forms == want and len(hc.quirk127_patterns()) >= 7
    assert len(length) == len(hc.LENGTH_SWEEP_B0) * 2 * len(want)
    assert {(k[1], k[2]) for k in length} == {(b0, m) for b0 in hc.LENGTH_SWEEP_B0 for m in (0, 1)}


@pytest.mark.parametrize("mode", MODES)
def test_every_record_kind_stands_at_every_phase(mode):
    """The corpus's name for itself, proven: each kind's sixteen records cover
    the sixteen values of hdr_off mod 16; gaps are 0-17 bytes; keys are
    non-zero with four distinct bytes; the two frames at the cap are whole."""
    c = hc.corpus(mode)
    assert c.wire_len < 64 << 20
    assert np.all(np.diff(c.hdr_off) > 0)
    body = c.kind_id >= 0
    seen = np.zeros((len(c.kinds), 16), bool)
    seen[c.kind_id[body], c.hdr_off[body] % 16] = True
    assert seen.all()
    assert np.bincount(c.kind_id[body], minlength=len(c.kinds)).tolist() == [16] * len(c.kinds)
    for f in np.nonzero(body)[0]:  # the bytes at each offset are the kind's header; keys as promised
        sweep, b0, mask, form, is_pat = c.kinds[c.kind_id[f]]
        h = int(c.hdr_off[f])
        hdr = hc.header_bytes(b0, mask, form, b"\1\2\3\4" if mask else b"")
        n = len(hdr) - (4 if mask else 0)
        assert bytes(c.wire[h:h + n]) == hdr[:n]
        if mask:
            key = bytes(c.wire[h + n:h + n + 4])
            assert 0 not in key and len(set(key)) == 4
    # the tail: the cap and cap + 1 complete, then the truncated records
    t = np.nonzero(~body)[0]
    assert t.tolist() == list(range(c.n - 5, c.n))
    for f, L in zip(t[:2], (hc.MAX_LEN, hc.MAX_LEN + 1)):
        hl = 14 if mode == hc.SERVER else 10
        assert bytes(c.wire[c.hdr_off[f] + 2:c.hdr_off[f] + 10]) == L.to_bytes(8, "big")
        assert c.hdr_off[f] + hl + L <= c.hdr_off[f + 1]


@pytest.mark.parametrize("mode", MODES)
def test_every_wserror_occurs_and_gaps_are_small(mode):
    c, e = hc.corpus(mode), hc.corpus_expected(mode)
    assert set(np.unique(e.err).tolist()) == {0, 1, 5, 6, 7}
    for code in (0, 5, 6, 7):  # err 1 needs the wire's end
        assert set((c.hdr_off[e.err == code] % 16).tolist()) == set(range(16)), code
    # good frames: a gap of 0-17 bytes to the next header, except behind a
    # pattern record (its room is fixed) -- gaps are legal and are there
    good = np.nonzero((e.err == 0) & (c.kind_id >= 0))[0]
    plain = np.array([not c.kinds[c.kind_id[f]][4] for f in good])
    gap = c.hdr_off[good + 1] - (e.off[good] + e.len[good])
    assert gap[plain].min() == 0 and gap[plain].max() == 17
    assert set(gap[plain].tolist()) == set(range(18))
    # flags: byte 0 | mask << 8 wherever two header bytes are inside the wire
    two = c.hdr_off + 2 <= c.wire_len
    assert two.all()
    assert np.array_equal(e.flags, c.wire[c.hdr_off].astype(np.int64) | ((c.wire[c.hdr_off + 1] >> 7).astype(np.int64) << 8))
    # error frames carry nothing
    bad = e.err != 0
    assert np.array_equal(e.off[bad], c.hdr_off[bad]) and not e.len[bad].any() and not e.key[bad].any()
    # every header length the mode accepts is among the good frames (a SERVER
    # takes unmasked frames only when empty: 2 bytes, or 10 with a 127-class 0)
    hl = (e.off - c.hdr_off)[e.err == 0]
    assert set(hl.tolist()) == ({2, 10, 6, 8, 14} if mode == hc.SERVER else {2, 4, 10})


def test_expect_agrees_with_the_golden_decode_vectors():
    """The vectors test_unpack_error_codes_match_reference runs on the device."""
    with open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")) as f:
        gold = json.load(f)
    ran = 0
    for c in gold["decode"]:
        data = bytes.fromhex(c["input_hex"])
        if "tail_gen" in c or not data or c["chunk"]:
            continue
        mode = hc.SERVER if c["mode"] == "SERVER" else hc.CLIENT
        want = c["expect_rets"][0]
        want = 0 if want == 8 else want  # CLOSE: the frame itself decodes fine
        err, off, length, key, flags = hc.expect(np.frombuffer(data, np.uint8), len(data), [0], 0, mode)
        if c["expect_frames"] and want == 0:
            fr = c["expect_frames"][0]
            assert err == 0, c["name"]
            assert length == fr["length"], c["name"]
            assert key == (int.from_bytes(bytes.fromhex(fr["maskey"]), "little") if fr["mask"] else 0), c["name"]
            assert off + length <= len(data), c["name"]
            got = hc.expect_full(np.frombuffer(data, np.uint8), len(data), [0], 0, mode)[5]
            assert got == bytes.fromhex(fr["payload_hex"]), c["name"]
        else:
            assert err == want and (off, length, key) == (0, 0, 0), c["name"]
        assert flags == ((data[0] | (data[1] >> 7) << 8) if len(data) >= 2 else 0), c["name"]
        ran += 1
    assert ran >= 15


def test_tail_records_are_what_their_names_say():
    hls = []
    for name, mode, frame, hl, err in hc.tail_records():
        got = hc.expect(np.frombuffer(frame, np.uint8), len(frame), [0], 0, mode)
        assert got[0] == err, name
        if err == 0:
            assert got[1] == hl and got[1] + got[2] == len(frame), name
            hls.append(hl)
    assert hls == [2, 4, 6, 8, 10, 14]
    # the truncation order of the reference: HDR1 rejects a non-FIN control byte
    # with one byte in hand; every other first byte waits for the second
    assert hc.expect(np.array([0x09], np.uint8), 1, [0], 0, hc.SERVER)[:2] == (7, 0)
    assert hc.expect(np.array([0x89], np.uint8), 1, [0], 0, hc.SERVER)[0] == 1
    assert hc.expect(np.array([0x09], np.uint8), 0, [0], 0, hc.SERVER) == (1, 0, 0, 0, 0)


def test_place_streams_puts_every_stream_at_its_phase():
    items = [(s, (3 * i + 5) % 16) for i, s in enumerate(hc.walk_streams().values())]
    wire, off, streams = hc.place_streams(items, n_streams=2 * len(items))
    assert len(off) == len(streams) + 1 and off[-1] == len(wire)
    for s, (a, b) in zip(streams, zip(off[:-1], off[1:])):
        assert wire[a:b] == s
    real = [i for i in range(len(streams)) if i % 2 == 0 and i < 2 * len(items) - 1]
    assert [off[i] % 16 for i in real] == [ph for _, ph in items]
    assert [streams[i] for i in real] == [s for s, _ in items]


def _walk_cases():
    return [(name, cap) for name in hc.walk_streams() for cap in hc.WALK_CAPS]


def test_the_walk_stream_list_is_the_issue_s():
    names = set(hc.walk_streams())
    assert {f"count_{n}" for n in (15, 16, 17, 31, 32, 33)} <= names
    assert {"close", "x16_0", "x16_125", "x64_bit63", "x64_max_plus_1", "one_byte", "empty"} <= names
    assert {f"cut_{k:02d}" for k in range(15)} <= names  # every byte of the 14-byte header
    assert hc.WALK_CAPS == (1, 15, 16, 17, 32, 33, 100)
    # what each special does to the oracle: it stops there, with the special recorded
    ws = hc.walk_streams()
    for name in ("x16_0", "x16_125", "x64_bit63", "x64_max_plus_1"):
        offs, used = hc.walk_expect(ws[name], 100)
        assert len(offs) == 3 and used == offs[2], name
    offs, used = hc.walk_expect(ws["close"], 100)
    assert len(offs) == 3 and used > offs[2] and used < len(ws["close"])
    for n in hc.WALK_COUNTS:
        offs, used = hc.walk_expect(ws[f"count_{n}"], 100)
        assert len(offs) == n and used == len(ws[f"count_{n}"])
    assert hc.walk_expect(ws["one_byte"], 100) == ([0], 0) and hc.walk_expect(ws["empty"], 100) == ([], 0)


@pytest.mark.parametrize("name", list(hc.walk_streams()))
def test_host_walk_matches_the_oracle(name):
    """kmws_find_headers == walk_expect: the offsets it records, how many, and
    the bytes it reports consumed, at every cap."""
    from kuma_amd import kmws
    stream = hc.walk_streams()[name]
    for cap in hc.WALK_CAPS:
        offs, used = kmws.find_headers(stream, cap=cap)
        assert (offs, used) == hc.walk_expect(stream, cap), (name, cap)
