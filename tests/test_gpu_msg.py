"""kmws_msg_index on the device against tests/msg_ref.py (pinned by
tests/test_msg_ref.py): the known answers, every scan shape around the block
size F (the constant kmws_msg_rule.hpp exports) and past one round of the
aggregate scans, messages and stream edges across blocks, the carry through
four batches, sums past 2^32, the contract (msg_cap, malformed arguments, an
empty batch), the real parse / gather / checks in front, the seeded fuzz, a graph
replay and the workspace guards.  Every call runs between guard regions
(msg_util.run_gpu)."""
import functools
import random

import numpy as np
import pytest

import msg_ref as mr
import msg_util as mu
import proto_ref as pr

pytestmark = pytest.mark.gpu

F = mu.block_frames()


# ---------------------------------------------------------------- known answers

@pytest.mark.parametrize("pos", [None, "dense"], ids=["pos_null", "pos_dense"])
def test_known_answers_as_one_batch(pos):
    streams, carries, recs, msg_of, first_of, after = mr.known_batch()
    got, want = mu.check(streams, pos=pos, carries=carries)
    assert want == (recs, msg_of, first_of, after)  # the model's answer is the typed one
    assert got["count"] == len(recs)


def test_known_answers_with_null_outputs_and_verdicts():
    streams, carries, _, _, _, _ = mr.known_batch()
    n = sum(len(s) for s in streams)
    utf8 = [(i * 7 + 1) % 4 for i in range(n)]
    proto = [(i * 5 + 3) % 11 for i in range(n)]
    mu.check(streams, carries=carries, utf8=utf8, proto=proto)
    mu.check(streams, carries=carries, utf8=utf8, outputs=False)
    # a gather that leaves the PING's payload elsewhere makes the message one run
    frames = [pr.fr(pr.T, 0, payload=b"ab"), pr.fr(pr.PING, payload=b"??"), pr.fr(pr.C, 1, payload=b"cd")]
    got, _ = mu.check([frames], pos=[100, 7, 102])
    assert got["recs"]["bits"][0] == mr.BEGIN | mr.END | mr.CONTIG


# ---------------------------------------------------------------- scan shapes

@functools.lru_cache(maxsize=None)
def pattern(n):
    """n frames: messages of 1-5 fragments, control frames with and without
    payload between them, and sprinkled in heads inside open messages, orphan
    CONTINUEs and reserved opcodes."""
    rng = random.Random(n)
    out = []
    while len(out) < n:
        out += pr._clean_message(rng, pr.R1, (0, 3))
    same = {}
    out = [same.setdefault(f, f) for f in out[:n]]  # a handful of objects, however long the list
    for p in range(5, n, 61):
        out[p] = rng.choice((pr.fr(pr.C, 1, payload=b"o"), pr.fr(pr.T, 0, payload=b"head"), pr.fr(5, 0), pr.fr(pr.C, 0),
                             pr.close(1000, b"bye"), pr.fr(pr.B, payload=b"x")))
    return out


def cut(frames, bounds):
    return [frames[a:b] for a, b in zip(bounds, bounds[1:])]


def mixed_carries(ns):
    kinds = (mr.ZERO, mr.carry(0x01, 5), mr.ZERO, mr.carry(0x42, (1 << 32) + 1))
    return [kinds[k & 3] for k in range(ns)]


SHAPES = [1, 63, 64, 65, F - 1, F, F + 1, 2 * F + 1, F * F + 3]


@pytest.mark.parametrize("n", SHAPES)
def test_scan_shape_one_stream(n):
    frames = pattern(n)
    mu.check([frames], one_stream=True, carries=[mr.carry(0x02, 9)])
    if n <= 2 * F + 1:
        mu.check([frames])  # the same through a stream_first of two entries


@pytest.mark.parametrize("n", SHAPES)
def test_scan_shape_one_stream_per_frame(n):
    mu.check(cut(pattern(n), list(range(n + 1))), carries=mixed_carries(n))


@pytest.mark.parametrize("n", SHAPES)
def test_scan_shape_streams_end_at_block_boundaries(n):
    bounds = list(range(0, n, F)) + [n]
    mu.check(cut(pattern(n), bounds), carries=mixed_carries(len(bounds) - 1))


@pytest.mark.parametrize("n", SHAPES)
def test_scan_shape_empty_streams_first_middle_last(n):
    a, b = n // 3, n - n // 4
    mu.check(cut(pattern(n), [0, 0, 0, a, a, a, a, b, n, n, n]), carries=mixed_carries(10))


def test_more_streams_than_frames():
    """The stream arrays are longer than the frame arrays: their blocks run too."""
    ns = 2 * F + 7
    bounds = [0] * (ns - 2) + [0, 1, 3]
    got, _ = mu.check(cut([pr.fr(pr.C, 1, payload=b"abc"), pr.fr(pr.T, 0, payload=b"de"), pr.fr(pr.PING)], bounds),
                      carries=mixed_carries(ns))
    assert got["count"] == 2 and got["carries"][ns - 4] == mixed_carries(ns)[ns - 4]


# ---------------------------------------------------------------- past one round of the aggregate scans

# A round of an aggregate scan takes F aggregates of F frames, four a lane.  F * F + 3 (above) puts one
# aggregate into round two: lane 0's first.  These put one into lane 1 of round two (1,029 aggregates), into
# lane 64, past a wave edge (1,281), and into round three.
ROUND_TWO_LANE_1 = F * F + 4 * F + 1
ROUND_SHAPES = [ROUND_TWO_LANE_1, (F + 256) * F + 1, 2 * F * F + 1]


@pytest.mark.parametrize("n", ROUND_SHAPES)
def test_scan_rounds_one_stream(n):
    assert -(-n // F) == {0: F + 5, 1: F + 257, 2: 2 * F + 1}[ROUND_SHAPES.index(n)]
    mu.check([pattern(n)], one_stream=True, carries=[mr.carry(0x02, 9)])


def test_scan_rounds_streams_end_at_block_boundaries():
    n = ROUND_TWO_LANE_1
    bounds = list(range(0, n, F)) + [n]
    mu.check(cut(pattern(n), bounds), carries=mixed_carries(len(bounds) - 1))


# the member's and the FIN's aggregates in round two: in lane 0, in lane 1, in lane 64 (past a wave edge)
@pytest.mark.parametrize("mid_block", [F + 1, F + 5, F + 257])
def test_message_open_across_rounds(mid_block):
    """Head in block F - 2, a member with payload in mid_block, FIN in the block
    after it, only PINGs between: the state of scan A and the 24-byte sum of scan
    B cross the round edge through the aggregate scans' running prefix."""
    n = (mid_block + 1) * F + 9
    head, mid, fin = (F - 2) * F + 10, mid_block * F + 5, (mid_block + 1) * F + 7
    frames = [pr.fr(pr.PING, payload=b"p")] * n
    frames[head] = pr.fr(pr.B, 0, payload=b"head")
    frames[mid] = pr.fr(pr.C, 0, payload=b"mid")
    frames[fin] = pr.fr(pr.C, 1, payload=b"tail!")
    got, _ = mu.check([frames], one_stream=True)
    r = got["recs"]
    assert got["count"] == 1 and (r["first"][0], r["last"][0], r["frames"][0], r["bytes"][0]) == (head, fin, 3, 12)
    assert r["bits"][0] == mr.BEGIN | mr.END  # the PINGs' payloads lie between
    frames[fin] = pr.fr(pr.PING)
    frames[fin + 1] = pr.fr(pr.C, 0, payload=b"x")  # the batch's last frame a member, the message left open
    got, _ = mu.check([frames], one_stream=True)
    assert got["carries"] == [mr.carry(0x02, 8)]


# ---------------------------------------------------------------- status bits and streams past round one

def empty_streams_batch(ns):
    """ns streams, all empty but the last two, and three frames: the first pass
    runs over stream_first alone and has ceil((ns + 1) / F) aggregates."""
    bounds = [0] * (ns - 2) + [0, 1, 3]
    return cut([pr.fr(pr.C, 1, payload=b"abc"), pr.fr(pr.T, 0, payload=b"de"), pr.fr(pr.PING)], bounds), bounds


NO_CARRY = b"\x7f" + bytes(15)  # test_malformed_carry_sets_status_bit_1


def empty_streams_carries(ns):
    """mixed_carries, and the first frame's stream comes with an open message: that CONTINUE|FIN ends it."""
    c = mixed_carries(ns)
    c[ns - 2] = mr.carry(0x01, 5)
    return c


def test_streams_past_one_round_without_frames():
    """Follows test_more_streams_than_frames: the status bits ride above the
    aggregates of round two; every empty stream's carry is copied and
    stream_msg_first holds (mu.check compares both)."""
    ns = F * F + 4 * F + 2
    assert -(-(ns + 1) // F) == F + 5
    streams, bounds = empty_streams_batch(ns)
    carries = empty_streams_carries(ns)
    got, _ = mu.check(streams, carries=carries)
    assert got["count"] == 2 and got["carries"][:ns - 2] == carries[:ns - 2]
    assert list(got["first_of"][[0, F * F, ns - 2, ns - 1, ns]]) == [0, 0, 0, 1, 2]
    # round two's lane 1; round one's last lane
    for x in (F * F + 4 * F + 1, F * F - 1):
        first = list(bounds)
        first[x] = first[x + 1] + 1  # descending
        assert mu.run_gpu(streams, carries=carries, stream_first=first)["status"] == 1, x
    for s in (F * F + 4 * F, F * F - 1):
        c = list(carries)
        c[s] = NO_CARRY
        assert mu.run_gpu(streams, carries=c)["status"] == 1, s


def test_streams_in_round_three_without_frames():
    ns = 2 * F * F + 5
    assert -(-(ns + 1) // F) == 2 * F + 1
    streams, bounds = empty_streams_batch(ns)
    carries = empty_streams_carries(ns)
    got = mu.run_gpu(streams, carries=carries)
    assert got["status"] == 0 and got["count"] == 2 and got["carries"][:ns - 2] == carries[:ns - 2]
    first = list(bounds)
    first[ns - 1] = first[ns] + 1  # the last aggregate
    assert mu.run_gpu(streams, carries=carries, stream_first=first)["status"] == 1
    c = list(carries)
    c[ns - 1] = NO_CARRY
    assert mu.run_gpu(streams, carries=c)["status"] == 1


# ---------------------------------------------------------------- across blocks

def test_message_open_across_blocks():
    """Head at frame 10, FIN at frame 2F + 7, only PINGs between: state and sums cross two block edges."""
    n = 2 * F + 9
    frames = [pr.fr(pr.PING, payload=b"p")] * n
    frames[10] = pr.fr(pr.B, 0, payload=b"head")
    frames[2 * F + 7] = pr.fr(pr.C, 1, payload=b"tail!")
    got, _ = mu.check([frames], one_stream=True)
    r = got["recs"]
    assert got["count"] == 1 and (r["first"][0], r["last"][0], r["frames"][0], r["bytes"][0]) == (10, 2 * F + 7, 2, 9)
    assert r["bits"][0] == mr.BEGIN | mr.END  # the PINGs' payloads lie between
    frames[2 * F + 7] = pr.fr(pr.PING)
    frames[2 * F + 8] = pr.fr(pr.C, 0, payload=b"x")  # the batch's last frame a member, the message left open
    got, _ = mu.check([frames], one_stream=True)
    assert got["carries"] == [mr.carry(0x02, 5)]


def test_nothing_leaks_across_a_stream_edge_at_a_block_edge():
    """A message ends in a stream's last frame, a block's last; the next stream
    starts the next block with a CONTINUE: an orphan, or a member of that stream's
    carried message."""
    n = F + 4
    frames = [pr.fr(pr.T, payload=b"m")] * n
    frames[F - 2] = pr.fr(pr.B, 0, payload=b"ab")
    frames[F - 1] = pr.fr(pr.C, 1, payload=b"c")
    frames[F] = pr.fr(pr.C, 1, payload=b"zz")
    got, _ = mu.check(cut(frames, [0, F, n]))
    assert got["msg_of"][F] == mr.NONE and got["first_of"][1] == F - 1
    got, _ = mu.check(cut(frames, [0, F, n]), carries=[mr.ZERO, mr.carry(0x01, 40)])
    r = got["recs"][F - 1]
    assert (r["stream"], r["first"], r["bytes"], r["prior"], r["bits"]) == (1, F, 2, 40, mr.END | mr.CONTIG)
    # the first stream left open at the block's last frame does not open the second
    frames[F - 1] = pr.fr(pr.C, 0, payload=b"c")
    got, _ = mu.check(cut(frames, [0, F, n]))
    assert got["msg_of"][F] == mr.NONE and got["carries"][0] == mr.carry(0x02, 3)


# ---------------------------------------------------------------- carry

def test_carry_chains_four_batches():
    streams = pr.fuzz_streams(seed=11, n_streams=150, data_lens=(0, 1, 7, 300))
    whole, _ = mu.check(streams)
    rng = random.Random(5)
    cuts = [sorted(rng.randrange(len(s) + 1) for _ in range(3)) for s in streams]
    carries, pieces, base = None, {}, 0
    for b in range(4):
        part = [s[([0] + c)[b]:(c + [len(s)])[b]] for s, c in zip(streams, cuts)]
        got, _ = mu.check(part, carries=carries)
        carries = got["carries"]
        # the batch's frame indices back to the whole batch's: per stream, shifted by its cut
        starts = np.cumsum([0] + [len(s) for s in streams])
        pstarts = np.cumsum([0] + [len(p) for p in part])
        for r in got["recs"]:
            s = int(r["stream"])
            first_whole = int(r["first"]) - int(pstarts[s]) + int(starts[s]) + ([0] + cuts[s])[b]
            pieces.setdefault((s, first_whole), r)
    assert carries == whole["carries"]
    # every message of the one-batch run: its pieces chain through prior, BEGIN and END appear once
    by_msg = {}
    for (s, first), r in sorted(pieces.items(), key=lambda kv: kv[0]):
        if r["bits"] & mr.BEGIN:
            by_msg[(s, first)] = [r]
            last_key = (s, first)
        else:
            assert last_key[0] == s
            by_msg[last_key].append(r)
    assert len(by_msg) == whole["count"]
    split = 0
    for w in whole["recs"]:
        ps = by_msg[(int(w["stream"]), int(w["first"]))]
        split += len(ps) > 1
        assert sum(int(p["bytes"]) for p in ps) == int(w["bytes"]) and sum(int(p["frames"]) for p in ps) == int(w["frames"])
        done = 0
        for p in ps:
            assert int(p["prior"]) == done and p["b0"] == w["b0"]
            done += int(p["bytes"])
        assert sum(bool(p["bits"] & mr.BEGIN) for p in ps) == 1
        assert sum(bool(p["bits"] & mr.END) for p in ps) == bool(w["bits"] & mr.END)
    assert split > 5  # the cuts do fall inside messages


def test_sums_past_2_to_32_without_memory():
    big = 0xFFFFFFF0
    frames = [pr.fr(pr.B, 0), pr.fr(pr.PING), pr.fr(pr.C, 0), pr.fr(pr.C, 1), pr.fr(pr.T)]
    lens = [big, 0, big, big, 5]
    p0 = (1 << 40) + 12345
    pos = [p0, p0 + big, p0 + big, p0 + 2 * big, p0 + 3 * big]
    for one in (False, True):
        got, _ = mu.check([frames], pos=pos, lens=lens, one_stream=one)
        r = got["recs"][0]
        assert int(r["bytes"]) == 3 * big > 1 << 33 and int(r["off"]) == p0 and r["bits"] == mr.BEGIN | mr.END | mr.CONTIG
    got, _ = mu.check([frames[:3]], pos=pos[:3], lens=lens[:3], carries=[mr.carry(0x02, (1 << 40) + 1)])
    assert got["carries"] == [mr.carry(0x02, 2 * big)]  # the head replaced the carried message
    got, _ = mu.check([frames[2:]], pos=pos[2:], lens=lens[2:], carries=[mr.carry(0x02, (1 << 40) + 1)])
    assert int(got["recs"]["prior"][0]) == (1 << 40) + 1


# ---------------------------------------------------------------- contract

def test_msg_cap_one_too_small_sets_status_bit_1():
    streams = pr.fuzz_streams(seed=2, n_streams=40)
    want = mr.walk(streams, mr.dense_pos(streams))
    need = len(want[0])
    assert need > 50
    got = mu.run_gpu(streams, msg_cap=need - 1)
    assert got["status"] == 1 and got["count"] == need
    got = mu.run_gpu(streams, msg_cap=need)
    mu.compare(got, want)
    got = mu.run_gpu(streams, msg_cap=0)
    assert got["status"] == 1 and got["count"] == need
    # a later call with room on the same workspace clears the status word
    keep = {}
    assert mu.run_gpu(streams, msg_cap=need - 1, keep=keep)["status"] == 1
    from kuma_amd import kmws
    import torch as T
    msgs = T.empty(need * 48, dtype=T.uint8, device="cuda")
    kmws.msg_index(keep["descs"], keep["fl"], msgs, keep["count"], keep["ws"], **{**keep["args"], "msg_cap": need})
    assert keep["ws"].status() == 0


def test_malformed_stream_first_sets_status_bit_1():
    streams = [[pr.fr(pr.T)] * 3, [pr.fr(pr.T)] * 2]
    assert mu.run_gpu(streams)["status"] == 0
    for bad in ([1, 3, 5], [0, 4, 3], [0, 3, 4], [0, 3, 6]):
        assert mu.run_gpu(streams, stream_first=bad)["status"] == 1, bad


def test_malformed_carry_sets_status_bit_1():
    streams = [[pr.fr(pr.T)], [], [pr.fr(pr.C, 1)]]
    ok = mr.carry(0x01, 3)
    assert mu.run_gpu(streams, carries=[mr.ZERO, ok, ok])["status"] == 0
    for bad in (b"\x01" + bytes(15), b"\x7f" + bytes(15), b"\x81\x00\x00\x01" + bytes(12), bytes(7) + b"\x01" + bytes(8)):
        for where in range(3):  # an empty stream's too
            c = [mr.ZERO, ok, ok]
            c[where] = bad
            assert mu.run_gpu(streams, carries=c)["status"] == 1, (bad, where)
    assert mu.run_gpu([[pr.fr(pr.T)]], carries=[b"\x05" + bytes(15)], one_stream=True)["status"] == 1
    # b[8..15] without an open message is not looked at
    assert mu.run_gpu(streams, carries=[bytes(8) + b"\x09" + bytes(7), ok, ok])["status"] == 0


def test_empty_batch_with_and_without_carries():
    c = [mr.carry(0x01, 7), mr.ZERO, mr.carry(0x42, 1 << 35)]
    got = mu.run_gpu([[], [], []], carries=c)
    assert got["count"] == 0 and list(got["first_of"]) == [0, 0, 0, 0] and got["carries"] == c
    got = mu.run_gpu([[], [], []])
    assert got["count"] == 0 and got["carries"] == [mr.ZERO] * 3
    got = mu.run_gpu([[]], one_stream=True, outputs=False)
    assert got["count"] == 0


# ---------------------------------------------------------------- behind the real front

def test_behind_unpack_gather_utf8_and_proto_check():
    """A masked server-mode wire through kmws_unpack_gather_utf8 and
    kmws_proto_check; the index gets pos = dst_off and both verdict arrays.  Every
    record with CONTIG is the message's payload at dst[off : off + bytes]."""
    import torch as T
    from kuma_amd import kmws
    streams = pr.fuzz_streams(seed=31, n_streams=120, data_lens=(0, 1, 7, 125, 126, 300))
    # text that is and is not UTF-8, in one frame and across fragments
    streams += [[pr.fr(pr.T, 0, payload="grü".encode()[:3]), pr.fr(pr.PING, payload=b"?"),
                 pr.fr(pr.C, 1, payload="grüß".encode()[3:])],
                [pr.fr(pr.T, payload=b"\xff\xfe"), pr.fr(pr.T, 0, payload=b"ok\xe2"), pr.fr(pr.C, 1, payload=b"\x82\xac")],
                [pr.fr(pr.T, 0, payload=b"bad\xc0"), pr.fr(pr.C, 0, payload=b"more"), pr.fr(pr.C, 1, payload=b"end")]]
    streams = [[f._replace(err=0) for f in s] for s in streams]  # a wire cannot carry the parser's verdict
    flat = [f for s in streams for f in s]
    n, ns = len(flat), len(streams)
    wire, hdr_off = bytearray(), []
    for i, f in enumerate(flat):
        hdr_off.append(len(wire))
        key = bytes([i & 0xFF, 0x80 | (i >> 8) & 0x7F, 0x33, 0xC4])
        wire += pr.wire_of([f], lambda _: key)
    total = len(wire)
    dev = "cuda"
    d_wire = T.from_numpy(np.frombuffer(bytes(wire) + b"\0" * (16 + -total % 16), dtype=np.uint8).copy()).to(dev)
    first = [int(x) for x in np.cumsum([0] + [len(s) for s in streams])]
    sf = T.tensor(first, dtype=T.int32, device=dev)
    desc = T.zeros((n, 2), dtype=T.int64, device=dev)
    flags = T.zeros(n, dtype=T.int16, device=dev)
    err = T.zeros(n, dtype=T.uint8, device=dev)
    utf8 = T.zeros(n, dtype=T.uint8, device=dev)
    proto = T.zeros(n, dtype=T.uint8, device=dev)
    cap_d = (sum(len(f.payload) for f in flat) + 15) // 16 * 16 + 16
    dst = T.full((cap_d,), 0x5A, dtype=T.uint8, device=dev)
    dst_off = T.zeros(n + 1, dtype=T.int64, device=dev)
    ws_g = kmws.Workspace(kmws.gather_utf8_workspace_size(n, cap_d, ns))
    kmws.unpack_gather_utf8(d_wire, T.tensor(hdr_off, dtype=T.int64, device=dev), kmws.SERVER, desc, flags, err, dst,
                            dst_off, utf8, ws_g, wire_len=total, stream_first=sf)
    e = err.cpu().numpy()
    assert ws_g.status() == (2 if e.any() else 0)
    # a frame whose header the parse rejects (a control frame without FIN or above 125 bytes) arrives with
    # len 0 and its flags as parsed: the model gets it the same way
    assert 0 < np.count_nonzero(e) < n // 4
    streams = [[f._replace(payload=b"") if e[first[k] + i] else f for i, f in enumerate(s)]
               for k, s in enumerate(streams)]
    flat = [f for s in streams for f in s]
    ws_p = kmws.Workspace(kmws.proto_workspace_size(n, ns))
    kmws.proto_check(d_wire, desc, flags, proto, ws_p, err=err, span=total, masked=True, rsv_allowed=pr.R1,
                     stream_first=sf)
    assert ws_p.status() == 0
    msgs = T.zeros(n * 48, dtype=T.uint8, device=dev)
    count = T.zeros(1, dtype=T.int32, device=dev)
    msg_of = T.zeros(n, dtype=T.int32, device=dev)
    ws_m = kmws.Workspace(kmws.msg_workspace_size(n, ns))
    kmws.msg_index(desc, flags, msgs, count, ws_m, pos=dst_off[:n], utf8=utf8, proto=proto, stream_first=sf,
                   msg_of=msg_of)
    assert ws_m.status() == 0
    pos = dst_off.cpu().numpy()
    u, p = utf8.cpu().numpy(), proto.cpu().numpy()
    assert list(pos[:n]) == mr.dense_pos(streams)
    want = mr.walk(streams, [int(x) for x in pos[:n]], utf8=[int(x) for x in u], proto=[int(x) for x in p])
    recs = msgs.cpu().numpy()[:int(count.item()) * 48].view(kmws.msg_dtype())
    mu.compare(dict(status=0, count=int(count.item()), recs=recs), want)
    assert np.array_equal(msg_of.cpu().numpy().view(np.uint32), np.array(want[1], dtype=np.uint32))
    out = dst.cpu().numpy().tobytes()
    contig = 0
    for k, r in enumerate(recs):
        members = [flat[i] for i in range(n) if want[1][i] == k]
        assert (r["utf8"], r["proto"]) == (u[r["last"]], p[r["last"]])
        if r["bits"] & mr.CONTIG:
            contig += 1
            assert out[int(r["off"]):int(r["off"] + r["bytes"])] == b"".join(f.payload for f in members), k
    assert 0 < contig < len(recs)
    assert {kmws.UTF8_OK, kmws.UTF8_BAD, kmws.UTF8_AFTER_BAD, kmws.UTF8_NOT_TEXT} <= set(int(x) for x in recs["utf8"])
    assert len(set(int(x) for x in recs["proto"])) > 3


# ---------------------------------------------------------------- fuzz, graph, guards

def test_fuzz():
    streams = pr.fuzz_streams(seed=20261, n_streams=3000)
    rng = random.Random(9)
    carries = [rng.choice((mr.ZERO, mr.ZERO, mr.carry(rng.choice((1, 2, 0x41)), rng.randrange(1 << 34)))) for _ in streams]
    n = sum(len(s) for s in streams)
    got, _ = mu.check(streams, carries=carries, utf8=[rng.randrange(4) for _ in range(n)],
                      proto=[rng.randrange(11) for _ in range(n)])
    assert got["count"] > 3000
    mu.check(streams, pos=None)


def test_capture_and_replay_in_a_graph():
    import torch as T
    from kuma_amd import kmws
    streams = pr.fuzz_streams(seed=3, n_streams=300)
    carries = mixed_carries(len(streams))
    want = mr.walk(streams, mr.dense_pos(streams), carries=carries)
    keep = {}
    mu.compare(mu.run_gpu(streams, carries=carries, keep=keep), want)
    k = keep
    T.cuda.synchronize()
    g = T.cuda.CUDAGraph()
    with T.cuda.graph(g):  # a linear chain of five kernel nodes
        kmws.msg_index(k["descs"], k["fl"], k["msgs"], k["count"], k["ws"], **k["args"])
    T.cuda.synchronize()
    for t in (k["msgs"], k["args"]["msg_of"], k["args"]["stream_msg_first"], k["args"]["carry_out"], k["count"]):
        t.fill_(0x6B)
    k["ws"].tensor.fill_(0xFF)
    T.cuda.synchronize()
    g.replay()
    T.cuda.synchronize()
    n, ns = len(want[1]), len(streams)
    got = dict(status=k["ws"].status(), count=int(k["count"][0].item()),
               recs=k["msgs"].cpu().numpy()[:len(want[0]) * 48].view(kmws.msg_dtype()),
               msg_of=k["args"]["msg_of"].cpu().numpy().view(np.uint32)[:n],
               first_of=k["args"]["stream_msg_first"].cpu().numpy().view(np.uint32)[:ns + 1],
               carries=[bytes(c) for c in k["args"]["carry_out"].cpu().numpy()])
    mu.compare(got, want)


@pytest.mark.parametrize("n,ns", [(1, 1), (F, 1), (F + 1, 3), (3, 2 * F + 7), (5 * F + 17, F + 2)])
def test_workspace_guards(n, ns):
    """The entry between two guard regions at exactly kmws_msg_workspace_size bytes
    (run_gpu checks both), and one byte less is refused."""
    import torch as T
    from kuma_amd import kmws
    frames = pattern(n)
    bounds = sorted(random.Random(ns).randrange(n + 1) for _ in range(ns - 1))
    mu.check(cut(frames, [0] + bounds + [n]), carries=mixed_carries(ns))
    need = kmws.msg_workspace_size(n, ns)
    ws = kmws.Workspace(need)
    ws.tensor = ws.tensor[:need - 1]
    fake = T.zeros(64, dtype=T.int64, device="cuda")
    st = kmws.lib().kmws_msg_index(fake.data_ptr(), fake.data_ptr(), None, None, None, n, fake.data_ptr(), ns, None,
                                   None, None, fake.data_ptr(), 0, fake.data_ptr(), None, ws.ptr, need - 1, None)
    assert st == kmws.ERR_BUFFER_TOO_SMALL
