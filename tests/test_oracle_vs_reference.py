"""The oracle (oracle/kmws_oracle.c, our restatement) against kuma's own compiled
WSHandler.cpp (oracle/ref_build.py -> oracle/_ref/libkmws_ref_O3.so and _O0.so).

Every test runs against both builds and compares every observable: each feed's
return code, the number of callbacks after each feed, all eleven fields of
Frame.key() and the caller's buffer after each feed (the in-place unmask
contract).  Nothing is excluded.  A handler its callback destroyed is not fed
again, on any backend (tests/ref_cases.py).

BUILDS_DISAGREE is the list the two builds' disagreements would go on: it may
hold 127-class length patterns only, and it is empty -- over everything below
the -O0 and the -O3 build agree byte for byte.

Skipped only where the reference libraries are absent (no reference checkout
at build time).  No GPU needed."""
import collections
import json
import os

import numpy as np
import pytest

import header_cases as hc
import pack_edge_cases as pe
import ref_cases as rc
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")))

# 127-class length patterns (the eight length bytes, hex) on which the -O0 and
# the -O3 build of the reference disagree.  None was found.
BUILDS_DISAGREE = []

OPTS = ("O3", "O0")
pytestmark = pytest.mark.skipif(any(orc.reference(o) is None for o in OPTS),
                                reason="oracle/_ref/libkmws_ref_O3.so / _O0.so not built "
                                       "(the reference checkout was absent when build() ran)")


@pytest.fixture(params=OPTS)
def ref(request):
    return orc.reference(request.param)


def same_run(a, b, what):
    assert a.rets == b.rets, (what, "return codes")
    assert a.counts == b.counts, (what, "callback counts")
    assert a.frames == b.frames, (what, "frames")
    assert a.buffers == b.buffers, (what, "caller's buffers")


def test_disagreement_list_is_empty():
    assert BUILDS_DISAGREE == []


# ------------------------------ the golden vectors ------------------------------
@pytest.mark.parametrize("c", GOLD["decode"], ids=lambda c: c["name"])
def test_golden_decode_through_reference(ref, c):
    run = rc.run_case(ref, c)
    same_run(rc.run_case(orc, c), run, c["name"])
    groups = list(run.groups)
    assert groups[0] == c["expect_rets"]
    assert len(run.frames) == len(c["expect_frames"])
    for got, exp in zip(run.frames, c["expect_frames"]):
        fin, rsv1, rsv2, rsv3, opcode, mask, plen, xpl64, maskey, length, payload = got
        assert (fin, rsv1, rsv2, rsv3, opcode, mask, length) == tuple(
            exp[k] for k in ("fin", "rsv1", "rsv2", "rsv3", "opcode", "mask", "length"))
        assert maskey.hex() == exp["maskey"]
        assert payload == (bytes.fromhex(exp["payload_hex"]) if "payload_hex" in exp
                           else rc.gen(exp["payload_gen"], exp["length"]))
    for g, step in zip(groups[1:], c.get("then", [])):
        assert g == step["expect_rets"]


@pytest.mark.parametrize("c", GOLD["encode"], ids=lambda c: c["name"])
def test_golden_encode_through_reference(ref, c):
    assert rc.encode_run(ref, c) == c["expect_hex"] == rc.encode_run(orc, c)


@pytest.mark.parametrize("c", GOLD["mask"], ids=lambda c: c["name"])
def test_golden_mask_through_reference(ref, c):
    assert rc.mask_run(ref, c) == c["expect_hex"] == rc.mask_run(orc, c)


# ------------------------------ the header corpus ------------------------------
@pytest.mark.parametrize("mode", [hc.CLIENT, hc.SERVER], ids=["client", "server"])
def test_header_corpus_expectations_identical(ref, mode):
    """expect_full of every record (256 first bytes x mask x the length forms,
    the 127-class quirk patterns, the cap and cap + 1, each at every byte
    phase) from the reference decoder = from the oracle."""
    c = hc.corpus(mode)
    want = hc.corpus_expected(mode)
    got = hc.Expected(c.wire, c.wire_len, c.hdr_off, mode, decoder=ref.Decoder)
    for name in ("err", "off", "len", "key", "flags"):
        bad = np.nonzero(getattr(got, name) != getattr(want, name))[0]
        assert bad.size == 0, (name, bad[:5], [c.kinds[c.kind_id[i]] for i in bad[:5]])
    assert got.payload == want.payload


def test_header_walk_expectations_identical(ref):
    for name, s in hc.walk_streams().items():
        for cap in hc.WALK_CAPS:
            assert hc.walk_expect(s, cap, ref.Decoder) == hc.walk_expect(s, cap), (name, cap)


def test_header_tail_records_identical(ref):
    """Every tail record cut at every byte, through both decoders."""
    for name, mode, frame, hl, err in hc.tail_records():
        for cut in range(len(frame) + 1):
            a = rc.run_stream(orc, mode, frame[:cut], 0)
            same_run(a, rc.run_stream(ref, mode, frame[:cut], 0), (name, cut))
        assert a.rets[-1] == err, name


def _pack_batches():
    for name, case in pe.CASES.items():
        if case.encode:
            yield name, case.build(True)
    for n in pe.COUNT_EDGES:
        yield f"count_{n}", pe.frame_count_batch(n, True)
    for ph in (0, 7, 15):
        yield f"phase_{ph}", pe.phase_batch(ph, True, mixed_masks=True)


def test_pack_edge_frame_lists_identical(ref):
    """The wire image the oracle gives for every encode batch of
    tests/pack_edge_cases.py = the reference's encodeFrameHeader + handleDataMask
    frame by frame."""
    for name, (src, offs, lens, flags, keys) in _pack_batches():
        wire, woff = orc.encode_batch(src, offs, lens, flags, keys)
        parts = []
        for o, n, fl, k in zip(offs, lens, flags, keys):
            key = int(k).to_bytes(4, "little")
            parts.append(rc.wire_frame(ref, int(fl) & 0xFF, (int(fl) >> 8) & 1, int(n), key,
                                       src[int(o):int(o) + int(n)].tobytes()))
        want = b"".join(parts)
        assert wire.tobytes() == want, name
        assert list(woff) == list(np.cumsum([0] + [len(p) for p in parts[:-1]])), name


# ------------------------------ encode and mask tables ------------------------------
def test_encode_header_table(ref):
    """All 256 first bytes (the 64 flag / opcode-bit combinations of the fixture
    among them) x mask x ENCODE_LENGTHS."""
    for row in rc.encode_table_full():
        c = rc.encode_case(*row)
        assert rc.encode_run(ref, c) == rc.encode_run(orc, c), c["name"]


def test_encode_ignores_plen_and_xpl(ref):
    """The length class comes from `length` alone."""
    import ctypes as C
    for L in rc.ENCODE_LENGTHS:
        h = orc.OrcHdr()
        h.fin, h.opcode, h.length, h.plen, h.xpl64 = 1, 2, L, 127, 0x0102030405060708
        a, b = (C.c_uint8 * 14)(), (C.c_uint8 * 14)()
        na = orc.lib().orc_encode_header(C.byref(h), a)
        nb = ref._lib.ref_encode_header(C.byref(h), b)
        assert (na, bytes(a[:na])) == (nb, bytes(b[:nb])), L


def test_mask_table(ref):
    """Every length 0..67 x phase 0..7 x three keys: phase 0 through the flat
    handleDataMask, the others through the KMBuffer-chain overload."""
    for key, n, ph in rc.mask_table_full():
        data = rc.mask_data(n, n)
        want = orc.mask_bytes(key, data, ph)
        assert ref.mask_bytes(key, data, ph) == want, (key.hex(), n, ph)
        assert want == bytes(b ^ key[(ph + i) & 3] for i, b in enumerate(data))


def test_mask_chains(ref):
    for key, segs in rc.chain_cases():
        assert ref.mask_chain(key, segs) == orc.mask_chain(key, segs), (key.hex(), [len(s) for s in segs])


def test_mask_numpy_in_place(ref):
    key = rc.MASK_KEYS[1]
    for ph in (0, 3):
        a = np.frombuffer(rc.mask_data(70001, 3), np.uint8).copy()
        b = a.copy()
        orc.mask(key, a, ph)
        ref.mask(key, b, ph)
        assert np.array_equal(a, b)


# ------------------------------ streaming state ------------------------------
@pytest.mark.parametrize("c", rc.streaming_cases(), ids=lambda c: c["name"])
def test_streaming_state(ref, c):
    same_run(rc.run_case(orc, c), rc.run_case(ref, c), c["name"])


def test_streaming_cases_reach_what_they_name():
    """The cases do what their names say (through the oracle: the test above
    ties it to the reference)."""
    runs = {c["name"]: rc.run_case(orc, c) for c in rc.streaming_cases()}
    assert runs["close_then_trailing_same_feed"].rets == [8, 5, 1]  # empty feed, state not HDR1: :279
    assert runs["cap_10MiB_unmasked"].rets == [0] and runs["cap_10MiB_masked_two_feeds"].rets == [1, 0]
    assert runs["cap_plus_1_masked"].rets == [6, 5, 0]
    assert runs["destroy_at_frame_0"].rets == [9] and runs["destroy_at_close"].rets == [9]
    assert len(runs["destroy_at_middle_frame"].frames) == 2
    assert runs["destroy_at_reassembled_frame"].rets == [1, 9]
    assert runs["payload_three_feeds_masked"].rets == [1, 1, 0]
    assert len(runs["payload_three_feeds_masked"].frames) == 2
    for k in range(1, 15):
        assert runs[f"header14_cut_at_{k:02d}"].rets == [1, 0, 0]
    for name, run in runs.items():
        if name.startswith("error_"):
            g = run.groups
            assert [r for r in g[0] if r != 1][0] in (6, 7) and g[1] == [5] and g[2] == [5] and g[3][-1] == 0 and g[4] == [0], name


# ------------------------------ fuzz ------------------------------
@pytest.fixture(scope="module")
def fuzz_oracle_runs():
    streams = rc.fuzz_streams()
    return streams, [rc.run_stream(orc, m, s, cut, dz) for m, s, cut, dz in streams]


def test_fuzz_is_informative(fuzz_oracle_runs):
    """The floors the seeded mix has to meet for its agreement to mean something."""
    streams, runs = fuzz_oracle_runs
    assert len(streams) == rc.FUZZ_STREAMS == 2000
    codes = collections.Counter(r for run in runs for r in run.rets)
    ends = collections.Counter(run.rets[-1] for run in runs)
    assert len(codes) >= 5, codes
    assert ends[0] >= 100 and ends[1] >= 100 and ends[5] + ends[6] + ends[7] >= 100, ends
    # reassembly: two feeds in a row left the decoder inside a payload (so the
    # second one's bytes were buffered) and a later feed completed that frame
    reassembled = 0
    for (mode, s, cut, dz), run in zip(streams, runs):
        d = orc.Decoder(mode)
        d.destroy_on = dz
        pend = 0  # consecutive feeds that ended inside a payload: from the second on, bytes are buffered
        hit = False
        step = cut if cut > 0 else max(1, len(s))
        for i in range(0, len(s), step):
            n0 = len(d.frames)
            ret = d.feed(bytearray(s[i:i + step]))
            hit |= pend >= 2 and len(d.frames) > n0
            pend = pend + 1 if ret == 1 and d.state == 4 else 0
            if ret == 9 or hit:
                break
        reassembled += hit
    assert reassembled >= 50, reassembled
    print(f"fuzz: {len(streams)} streams, {sum(len(r.rets) for r in runs)} feeds, return codes {dict(codes)}, "
          f"stream ends {dict(ends)}, reassembly in {reassembled} streams")


def test_fuzz_against_reference(ref, fuzz_oracle_runs):
    streams, runs = fuzz_oracle_runs
    for i, ((mode, s, cut, dz), want) in enumerate(zip(streams, runs)):
        same_run(want, rc.run_stream(ref, mode, s, cut, dz), f"stream {i} mode {mode} cut {cut} destroy_on {dz}")
