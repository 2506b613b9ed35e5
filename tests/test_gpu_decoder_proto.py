"""kmws_decoder_set_proto_check on the host path with masking: SERVER-mode
handlers fed masked frames through kmws_decoder_feed, through the deferred feed
with kmws_rx_batch_flush, and with kmws_rx_batch_submit + kmws_rx_batch_poll;
the protocol check and the UTF-8 check both on.  Per delivered frame the
protocol verdict equals tests/proto_ref.py's and the UTF-8 verdict
tests/utf8_ref.py's on the same stream -- a CLOSE whose masked reason is not
UTF-8 included --, and payloads and return codes equal those of the same feed
with both checks off."""
import random

import pytest

import proto_ref as pr
import utf8_ref as ref
from kuma_amd import kmws

pytestmark = pytest.mark.gpu

ROUTES = ("feed", "flush", "poll")


def run(route, wire, chunk, on, rsv_allowed):
    h = kmws.WSHandler(kmws.SERVER)
    if on:
        h.set_proto_check(True, rsv_allowed)
        h.setUtf8Check(True)
    got = []

    def cb(hd, p):
        b0 = (hd.fin << 7) | (hd.rsv1 << 6) | (hd.rsv2 << 5) | (hd.rsv3 << 4) | hd.opcode
        got.append((b0, p, h.last_frame_proto(), hd.utf8))

    h.setFrameCallback(cb)
    rcs, outside = [], [h.last_frame_proto()]
    cuts = [wire[o:o + chunk] for o in range(0, len(wire), chunk)] if chunk else [wire]
    if route == "feed":
        for c in cuts:
            rcs.append(h.handleData(c))
            outside.append(h.last_frame_proto())
    else:
        b = kmws.RxBatch()
        for c in cuts:
            rcs.append(h.handleDataDeferred(b, c))
            outside.append(h.last_frame_proto())
            if route == "poll":
                b.submit()
        if route == "poll":
            b.poll(wait=True)
        else:
            b.flush()
        assert b.pending() == 0 and b.inflight() == 0
        outside.append(h.last_frame_proto())
    assert not any(outside)
    return rcs, got


def check_stream(frames, rsv_allowed=0, chunk=0, seed=1):
    rng = random.Random(seed)
    keys = [bytes(rng.randrange(256) for _ in range(4)) for _ in frames]
    wire = pr.wire_of(frames, lambda i: keys[i])
    delivered = pr.deliverable(frames)
    want_proto = pr.judge(frames, rsv_allowed)[0][:len(delivered)]
    want_utf8, _ = ref.validate_stream([(f.b0, f.payload) for f in delivered])
    for route in ROUTES:
        rc_on, got_on = run(route, wire, chunk, True, rsv_allowed)
        rc_off, got_off = run(route, wire, chunk, False, rsv_allowed)
        assert [(g[0], g[1]) for g in got_on] == [(f.b0, f.payload) for f in delivered], route
        assert [g[2] for g in got_on] == want_proto, (route, [g[2] for g in got_on], want_proto)
        assert [g[3] for g in got_on] == list(want_utf8), (route, [g[3] for g in got_on], want_utf8)
        assert [(g[0], g[1]) for g in got_off] == [(g[0], g[1]) for g in got_on] and rc_on == rc_off, route
        assert all(g[2] == 0 and g[3] == 0 for g in got_off), route
    return want_proto, list(want_utf8)


EURO = "€".encode()

CASES = [
    # a text message whose code point straddles two fragments, a PING between, then a CLOSE with a good reason
    ([pr.fr(pr.T, 0, payload=b"ab" + EURO[:1]), pr.fr(pr.PING, payload=b"?"), pr.fr(pr.C, 1, payload=EURO[1:] + b"!"),
      pr.close(1000, "tschüß".encode())], 0),
    # bad UTF-8 in a text message is the UTF-8 check's business (1007), not a protocol error
    ([pr.fr(pr.T, payload=b"a\xffb"), pr.fr(pr.B, payload=b"\xff" * 40), pr.fr(pr.T, payload=b"fine")], 0),
    # a CLOSE whose masked reason ends inside a code point
    ([pr.fr(pr.T, payload=b"hello"), pr.close(1000, b"bye " + EURO[:2])], 0),
    # a CLOSE with a code that may not be sent, a one-byte CLOSE
    ([pr.fr(pr.B, payload=b"\0" * 200), pr.close(1005, b"no status")], 0),
    ([pr.fr(8, payload=b"\x03")], 0),
    # sequence errors; the frames behind them are still delivered, as AFTER_FAIL
    ([pr.fr(pr.C, 1, payload=b"stray"), pr.fr(pr.T, payload=b"t")], 0),
    ([pr.fr(pr.T, 0, payload=b"one"), pr.fr(pr.T, 1, payload=b"two"), pr.fr(pr.C, 1, payload=b"three")], 0),
    ([pr.fr(3, payload=b"reserved"), pr.fr(pr.PING), pr.close(1000)], 0),
    # RSV1 negotiated and not
    ([pr.fr(pr.T, rsv=pr.R1, payload=b"\xf2\x48\xcd"), pr.fr(pr.T, rsv=pr.R2, payload=b"x")], pr.R1),
    ([pr.fr(pr.T, rsv=pr.R1, payload=b"\xf2\x48\xcd"), pr.fr(pr.T, payload=b"x")], 0),
]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_cases_through_every_route(k):
    frames, rsv = CASES[k]
    for chunk in (0, 7):
        proto, utf8 = check_stream(frames, rsv, chunk, seed=k)
    if k == 2:
        assert proto == [0, pr.CLOSE_REASON] and utf8 == [ref.OK, ref.NOT_TEXT]
    if k == 1:
        assert proto == [0, 0, 0] and utf8 == [ref.BAD, ref.NOT_TEXT, ref.OK]


def test_fuzz_streams_through_every_route():
    seen = set()
    for k, s in enumerate(pr.fuzz_streams(seed=91, n_streams=40, data_lens=(0, 1, 7, 130))):
        s = s[:next((i for i, f in enumerate(s) if f.err), len(s))]
        proto, _ = check_stream(s, pr.R1, chunk=(0, 64)[k & 1], seed=k)
        seen.update(proto)
    assert len(seen) >= 6
