"""kmws_proto_check on the device against tests/proto_ref.py (pinned by
tests/test_proto_ref.py): the known answers masked and plain at every payload
alignment, every scan shape around the block size F (the constant
kmws_proto_rule.hpp exports) and past one round of the aggregate scan, sequences
that must hold across blocks, the carry between two calls, err, the real header
parse in front, the contract, a payload past 2^32, and the seeded fuzz."""
import functools
import random

import numpy as np
import pytest

import proto_ref as pr
import proto_util as pu

pytestmark = pytest.mark.gpu

F = pu.block_frames()


def check(streams, rsv_allowed=0, carry_in=None, use_err=True, **kw):
    b = pr.device_batch(streams, **{k: kw.pop(k) for k in ("masked", "key_of", "align", "pad_end") if k in kw})
    masked = bool(kw.pop("masked_call", False))
    out, states, st = pu.run_gpu(b, masked=masked, rsv_allowed=rsv_allowed, carry_in=carry_in, use_err=use_err, **kw)
    want, want_states = pu.expect(streams, rsv_allowed, carry_in, use_err)
    assert st == 0
    bad = np.nonzero(out != want)[0]
    assert bad.size == 0, (bad[:10], out[bad[:10]], want[bad[:10]])
    assert np.array_equal(states, want_states)
    return out


# ---------------------------------------------------------------- known answers

def known_groups():
    groups = {}
    for name, rsv, frames, verdicts, _ in pr.KNOWN:
        groups.setdefault(rsv, []).append((frames, verdicts))
    return groups


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("zero_key", [False, True], ids=["keys", "key0"])
def test_known_answers(masked, zero_key):
    key_of = (lambda i: b"\0\0\0\0") if zero_key else None
    for rsv, cases in known_groups().items():
        streams = [frames for frames, _ in cases]
        typed = [v for _, verdicts in cases for v in verdicts]
        for align in range(16):
            # pad_end = 0: the last CLOSE payload ends exactly at the span
            out = check(streams, rsv, masked=masked, masked_call=masked, key_of=key_of, align=align, pad_end=0)
            assert list(out) == typed


def test_masked_flag_decides_how_the_body_is_read():
    """The same masked bytes read as plain give another code: the key is applied iff payload_masked."""
    s = [[pr.close(1000, b"bye")]]
    b = pr.device_batch(s, masked=True, key_of=lambda i: b"\x55\xaa\x0f\xf0")
    assert pu.run_gpu(b, masked=True)[0][0] == pr.OK
    assert pu.run_gpu(b, masked=False)[0][0] == pr.CLOSE_PAYLOAD


# ---------------------------------------------------------------- scan shapes

@functools.lru_cache(maxsize=None)
def pattern(n, single):
    """n frames: clean messages of 1-5 fragments with control frames between,
    valid CLOSEs and violations sprinkled in (for one long stream: a single
    violation at 90 %, so the states before it scan across every block)."""
    rng = random.Random(n)
    out = []
    while len(out) < n:
        out += pr._clean_message(rng, 0, (0, 3))
    same = {}
    out = [same.setdefault(f, f) for f in out[:n]]  # a handful of objects, however long the list
    if single:
        if n > 10:
            out[n * 9 // 10] = pr.fr(3)
    else:
        for p in range(700, n, 7919):
            out[p] = rng.choice((pr.fr(11), pr.close(1000, b"bye"), pr.close(1005), pr.fr(pr.PING, 0),
                                 pr.close(1000, b"\x80")))
    return out


def cut(frames, bounds):
    return [frames[a:b] for a, b in zip(bounds, bounds[1:])]


SHAPES = [1, 63, 64, 65, F - 1, F, F + 1, 2 * F + 1, F * F + 3]


@pytest.mark.parametrize("n", SHAPES)
def test_scan_shape_one_stream(n):
    frames = pattern(n, True)
    check([frames], one_stream=True)
    if n <= 2 * F + 1:
        check([frames])  # the same through a stream_first of two entries


@pytest.mark.parametrize("n", SHAPES)
def test_scan_shape_one_stream_per_frame(n):
    frames = pattern(n, False)
    check(cut(frames, list(range(n + 1))))


@pytest.mark.parametrize("n", SHAPES)
def test_scan_shape_streams_end_at_block_boundaries(n):
    frames = pattern(n, False)
    check(cut(frames, list(range(0, n, F)) + [n]))


@pytest.mark.parametrize("n", SHAPES)
def test_scan_shape_empty_streams_first_middle_last(n):
    frames = pattern(n, False)
    a, b = n // 3, n - n // 4
    check(cut(frames, [0, 0, 0, a, a, a, a, b, n, n, n]))


def test_more_streams_than_frames():
    """The stream arrays are longer than the frame arrays: their blocks run too."""
    ns = 2 * F + 7
    bounds = [0] * (ns - 2) + [0, 1, 3]
    carry = np.array([k & 3 for k in range(ns)], dtype=np.uint8)
    check(cut([pr.fr(pr.C, 1), pr.fr(pr.T), pr.fr(pr.PING)], bounds), carry_in=carry)


# ---------------------------------------------------------------- past one round of the aggregate scan

# A round of the aggregate scan takes F aggregates of F frames, four a lane.  F * F + 3 (above) puts one
# aggregate into round two: lane 0's first.  These put one into lane 1 of round two (1,029 aggregates), into
# lane 64, past a wave edge (1,281), and into round three.
ROUND_TWO_LANE_1 = F * F + 4 * F + 1
ROUND_SHAPES = [ROUND_TWO_LANE_1, (F + 256) * F + 1, 2 * F * F + 1]


@pytest.mark.parametrize("n", ROUND_SHAPES)
def test_scan_rounds_one_stream(n):
    """The stream comes with an open message, which frame 0 ends."""
    assert -(-n // F) == {0: F + 5, 1: F + 257, 2: 2 * F + 1}[ROUND_SHAPES.index(n)]
    frames = [pr.fr(pr.C, 1)] + pattern(n - 1, True)
    out = check([frames], one_stream=True, carry_in=[pr.OPEN])
    assert out[0] == pr.OK and not out[:(n - 1) * 9 // 10].any()


def test_scan_rounds_streams_end_at_block_boundaries():
    n = ROUND_TWO_LANE_1
    frames = pattern(n, False)
    check(cut(frames, list(range(0, n, F)) + [n]))


# the stray frame's aggregate in round two: lane 0's second, lane 1's second, lane 64's second (past a wave edge)
@pytest.mark.parametrize("stray_block", [F + 1, F + 5, F + 257])
def test_message_open_across_rounds(stray_block):
    """A message opened in block F - 2 is still open in the stray head's block,
    past the round edge: that head is a sequence error only because the state
    arrived through the aggregate scan's running prefix.  FAILED then reaches the
    last block.  The same with a CLOSE before the edge and data behind it."""
    n = (stray_block + 2) * F + 8
    head, stray = (F - 2) * F + 10, stray_block * F + 5
    frames = [pr.fr(pr.PING)] * n
    frames[head] = pr.fr(pr.T, 0)
    frames[stray] = pr.fr(pr.T, 0)
    out = check([frames], one_stream=True)
    assert not out[:stray].any() and out[stray] == pr.INTERLEAVED and (out[stray + 1:] == pr.AFTER_FAIL).all()
    assert pu.expect([frames])[1][0] == pr.FAILED
    frames[head] = pr.close(1000, b"bye")
    frames[stray] = pr.fr(pr.T)
    out = check([frames], one_stream=True)
    assert not out[:head + 1].any() and (out[head + 1:] == pr.AFTER_CLOSE).all()
    assert pu.expect([frames])[1][0] == pr.CLOSED


# ---------------------------------------------------------------- status bits and streams past round one

def empty_streams_batch(ns):
    """ns streams, all empty but the last two, and three frames: the first pass
    runs over stream_first alone and has ceil((ns + 1) / F) aggregates."""
    bounds = [0] * (ns - 2) + [0, 1, 3]
    return cut([pr.fr(pr.C, 1), pr.fr(pr.T), pr.fr(pr.PING)], bounds), bounds


def test_streams_past_one_round_without_frames():
    """Follows test_more_streams_than_frames: the status bits ride above the
    aggregates of round two, and every empty stream's carry is copied."""
    ns = F * F + 4 * F + 2
    assert -(-(ns + 1) // F) == F + 5
    streams, bounds = empty_streams_batch(ns)
    carry = np.array([k & 3 for k in range(ns)], dtype=np.uint8)
    check(streams, carry_in=carry)
    b = pr.device_batch(streams)
    # (index, in words): round two's lane 1; round one's last lane
    for x in (F * F + 4 * F + 1, F * F - 1):
        first = list(bounds)
        first[x] = first[x + 1] + 1  # descending
        b["stream_first"] = first
        assert pu.run_gpu(b, carry_in=carry)[2] == 1, x
    b["stream_first"] = bounds
    for s in (F * F + 4 * F, F * F - 1):
        c = carry.copy()
        c[s] = 7  # no state
        assert pu.run_gpu(b, carry_in=c)[2] == 1, s
    assert pu.run_gpu(b, carry_in=carry)[2] == 0


def test_streams_in_round_three_without_frames():
    ns = 2 * F * F + 5
    assert -(-(ns + 1) // F) == 2 * F + 1
    streams, bounds = empty_streams_batch(ns)
    carry = np.array([k & 3 for k in range(ns)], dtype=np.uint8)
    b = pr.device_batch(streams)
    out, states, st = pu.run_gpu(b, carry_in=carry)
    assert st == 0 and np.array_equal(states[:ns - 2], carry[:ns - 2])  # the empty streams' carries, copied
    first = list(bounds)
    first[ns - 1] = first[ns] + 1  # the last aggregate
    b["stream_first"] = first
    assert pu.run_gpu(b, carry_in=carry)[2] == 1
    b["stream_first"] = bounds
    c = carry.copy()
    c[ns - 1] = 7
    assert pu.run_gpu(b, carry_in=c)[2] == 1


# ---------------------------------------------------------------- across blocks

def test_message_open_across_blocks():
    n = 2 * F + 8
    frames = [pr.fr(pr.PING)] * n
    frames[10] = pr.fr(pr.T, 0)
    frames[2 * F + 5] = pr.fr(pr.C, 1)
    frames[2 * F + 7] = pr.fr(pr.C, 1)
    out = check([frames], one_stream=True)
    assert not out[:2 * F + 7].any() and out[2 * F + 7] == pr.CONTINUATION


def test_failure_reaches_the_streams_last_block_and_not_the_next_stream():
    n = 3 * F
    frames = [pr.fr(pr.T)] * n
    frames[3] = pr.fr(3)
    end = 2 * F + 10
    out = check(cut(frames, [0, end, n]))
    assert out[3] == pr.OPCODE and (out[4:end] == pr.AFTER_FAIL).all() and not out[end:].any()


@pytest.mark.parametrize("stream_ends_with_block", [False, True])
def test_close_as_a_blocks_last_frame(stream_ends_with_block):
    n = 2 * F
    frames = [pr.fr(pr.B)] * n
    frames[F - 1] = pr.close(1001, b"going away")
    out = check(cut(frames, [0, F if stream_ends_with_block else F + 5, n]))
    assert out[F - 1] == pr.OK
    assert (out[F:F + 5] == (pr.OK if stream_ends_with_block else pr.AFTER_CLOSE)).all()


# ---------------------------------------------------------------- carry

def carry_stream():
    rng = random.Random(40)
    s = []
    while len(s) < 40:
        s += pr._clean_message(rng, pr.R1, (0, 2))
    s = s[:40]
    s[33] = pr.close(1000, b"done")
    return s


@pytest.mark.parametrize("state", [pr.IDLE, pr.OPEN, pr.CLOSED, pr.FAILED])
def test_carry_chains_two_calls_at_every_split(state):
    s = carry_stream()
    b = pr.device_batch([s])
    whole, end, st = pu.run_gpu(b, rsv_allowed=pr.R1, carry_in=[state], one_stream=True)
    want, want_end = pu.expect([s], pr.R1, [state])
    assert st == 0 and np.array_equal(whole, want) and end[0] == want_end[0]
    for k in range(len(s) + 1):
        o1, c1, st1 = pu.run_gpu(b, rsv_allowed=pr.R1, carry_in=[state], one_stream=True, lo=0, hi=k)
        o2, c2, st2 = pu.run_gpu(b, rsv_allowed=pr.R1, carry_in=[int(c1[0])], one_stream=True, lo=k, hi=len(s))
        assert st1 == 0 and st2 == 0
        assert np.array_equal(np.concatenate([o1, o2]), whole), k
        assert c2[0] == end[0], k


def test_carry_byte_that_is_no_state_sets_status_bit_1():
    b = pr.device_batch([[pr.fr(pr.T)], [], [pr.fr(pr.T)]])
    assert pu.run_gpu(b, carry_in=[0, 1, 3])[2] == 0
    assert pu.run_gpu(b, carry_in=[0, 1, 7])[2] == 1
    assert pu.run_gpu(b, carry_in=[0, 7, 0])[2] == 1  # an empty stream's too
    assert pu.run_gpu(pr.device_batch([[pr.fr(pr.T)]]), carry_in=[4], one_stream=True)[2] == 1


# ---------------------------------------------------------------- err

def test_err_gives_header_then_after_fail_and_null_err_ignores_it():
    s = [[pr.fr(pr.T), pr.fr(pr.B, err=6), pr.fr(pr.T), pr.fr(pr.C, 1)], [pr.fr(pr.T, err=1)], [pr.fr(pr.T)]]
    out = check(s)
    assert list(out) == [0, pr.HEADER, pr.AFTER_FAIL, pr.AFTER_FAIL, pr.HEADER, 0]
    out = check(s, use_err=False)  # judged from flags and len alone
    assert list(out) == [0, 0, 0, pr.CONTINUATION, 0, 0]


# ---------------------------------------------------------------- behind the real parse

def test_composes_with_unpack_headers():
    """A server-mode wire through kmws_unpack_headers; its out_desc, out_flags and
    out_err go straight in (the wire is still masked)."""
    import torch as T
    from kuma_amd import kmws
    streams = [[pr.fr(pr.T, 0, payload=b"he"), pr.fr(pr.PING, payload=b"?"), pr.fr(pr.C, 1, payload=b"llo"),
                pr.close(1000, "grüß".encode())],
               [pr.fr(pr.B, 0, payload=b"\1" * 300), pr.fr(pr.C, 1, payload=b"tail"), pr.fr(pr.T, payload=b"x")],
               [pr.fr(pr.T, payload=b"ok"), pr.close(1000, b"\xe2\x82"), pr.fr(pr.T, payload=b"late")],
               [pr.fr(pr.T, rsv=pr.R1, payload=b"zz"), pr.fr(5, payload=b"r"), pr.close(1001)]]
    flat = [f for s in streams for f in s]
    unmasked = 5  # a frame with payload and no mask: the server-mode parse rejects its header
    wire, hdr_off = bytearray(), []
    for i, f in enumerate(flat):
        hdr_off.append(len(wire))
        key = None if i == unmasked else bytes([i + 1, 0x80 | i, 0x33, 0xC4])
        wire += pr.wire_of([f], (lambda _: key) if key else None)
    n = len(flat)
    d_wire = T.from_numpy(np.frombuffer(bytes(wire) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    desc = T.zeros((n, 2), dtype=T.int64, device="cuda")
    flags = T.zeros(n, dtype=T.int16, device="cuda")
    err = T.zeros(n, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(kmws.lib().kmws_unpack_workspace_size())
    kmws.unpack_headers(d_wire, T.tensor(hdr_off, dtype=T.int64, device="cuda"), kmws.SERVER, desc, flags, err, ws,
                        wire_len=len(wire))
    first = np.cumsum([0] + [len(s) for s in streams])
    out = T.full((n,), 0xEE, dtype=T.uint8, device="cuda")
    pws = kmws.Workspace(kmws.proto_workspace_size(n, len(streams)))
    kmws.proto_check(d_wire, desc, flags, out, pws, err=err, span=len(wire), masked=True, rsv_allowed=pr.R1,
                     stream_first=T.tensor(first, dtype=T.int32, device="cuda"))
    assert pws.status() == 0
    e = err.cpu().numpy()
    assert e[unmasked] != 0 and np.count_nonzero(e) == 1
    want, _ = pu.expect([[f._replace(err=int(e[i + first[k]])) for i, f in enumerate(s)]
                         for k, s in enumerate(streams)], pr.R1)
    assert list(out.cpu().numpy()) == list(want)
    assert list(want) == [0, 0, 0, 0, 0, pr.HEADER, pr.AFTER_FAIL, 0, pr.CLOSE_REASON, pr.AFTER_FAIL, 0, pr.OPCODE,
                          pr.AFTER_FAIL]


# ---------------------------------------------------------------- contract

def test_close_payload_past_span_sets_status_bit_1():
    s = [[pr.fr(pr.T, payload=b"x" * 50), pr.close(1000, b"bye")]]
    b = pr.device_batch(s, pad_end=0)
    assert b["off"][1] + b["len"][1] == len(b["base"])
    assert pu.run_gpu(b)[2] == 0
    assert pu.run_gpu(b, span=len(b["base"]) - 1)[2] == 1
    assert pu.run_gpu(b, span=b["off"][1] - 1)[2] == 1  # the offset itself past the span
    # other frames' descriptors are not looked at: a data frame far outside changes nothing
    b["off"][0] = 1 << 40
    out, _, st = pu.run_gpu(b)
    assert st == 0 and list(out) == [0, 0]
    # a later clean call on the same workspace clears the status word
    keep = {}
    assert pu.run_gpu(b, span=len(b["base"]) - 1, keep=keep)[2] == 1
    from kuma_amd import kmws
    kmws.proto_check(keep["base"], keep["descs"], keep["fl"], keep["out"], keep["ws"], err=keep["err"],
                     span=len(b["base"]), stream_first=keep["sf"])
    assert keep["ws"].status() == 0


def test_malformed_stream_first_sets_status_bit_1():
    b = pr.device_batch([[pr.fr(pr.T)] * 3, [pr.fr(pr.T)] * 2])
    assert pu.run_gpu(b)[2] == 0
    for bad in ([1, 3, 5], [0, 4, 3], [0, 3, 4], [0, 3, 6]):
        b["stream_first"] = bad
        assert pu.run_gpu(b)[2] == 1, bad


def test_empty_batch_copies_the_carries():
    out, states, st = pu.run_gpu(pr.device_batch([[], [], []]), carry_in=[1, 3, 2])
    assert out.size == 0 and list(states) == [1, 3, 2]


def test_capture_and_replay_in_a_graph():
    import torch as T
    from kuma_amd import kmws
    streams = pr.fuzz_streams(seed=3, n_streams=300)
    b = pr.device_batch(streams, masked=True)
    keep = {}
    out, states, st = pu.run_gpu(b, masked=True, rsv_allowed=pr.R1, keep=keep)
    want, want_states = pu.expect(streams, pr.R1)
    assert st == 0 and np.array_equal(out, want)
    k = keep
    T.cuda.synchronize()
    g = T.cuda.CUDAGraph()
    with T.cuda.graph(g):  # a linear chain of three kernel nodes
        kmws.proto_check(k["base"], k["descs"], k["fl"], k["out"], k["ws"], err=k["err"], masked=True,
                         span=len(b["base"]), rsv_allowed=pr.R1, stream_first=k["sf"], carry_out=k["co"])
    T.cuda.synchronize()
    k["out"].fill_(0xEE)
    k["co"].fill_(0xEE)
    k["ws"].tensor.fill_(0xFF)
    T.cuda.synchronize()
    g.replay()
    T.cuda.synchronize()
    assert k["ws"].status() == 0
    assert np.array_equal(k["out"].cpu().numpy()[:len(want)], want)
    assert np.array_equal(k["co"].cpu().numpy()[:, 0], want_states)


# ---------------------------------------------------------------- far offset

def test_close_payload_past_4_gib():
    import torch as T
    from kuma_amd import kmws
    span = (1 << 32) + 8192
    base = T.empty(span, dtype=T.uint8, device="cuda")  # otherwise untouched: nothing else may be read
    key = bytes([0x11, 0x22, 0x33, 0x44])
    bodies = [pr.close(1000, "far €".encode()), pr.close(1000, b"far \xe2\x82")]
    offs = [(1 << 32) + 101, (1 << 32) + 4099]
    for f, o in zip(bodies, offs):
        base[o:o + len(f.payload)] = T.from_numpy(np.frombuffer(pr.mask_bytes(f.payload, key), dtype=np.uint8).copy()).cuda()
    frames = [pr.fr(pr.T, payload=b"x" * 7), bodies[0], bodies[1]]
    descs = kmws.make_descs(np.array([0] + offs, dtype=np.int64), np.array([len(f.payload) for f in frames]),
                            np.full(3, int.from_bytes(key, "little"), dtype=np.int64))
    fl = T.tensor([f.b0 | 0x100 for f in frames], dtype=T.int16, device="cuda")
    out = T.full((3,), 0xEE, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(kmws.proto_workspace_size(3, 2))
    kmws.proto_check(base, descs, fl, out, ws, span=span, masked=True,
                     stream_first=T.tensor([0, 2, 3], dtype=T.int32, device="cuda"))
    assert ws.status() == 0
    assert list(out.cpu().numpy()) == [pr.OK, pr.OK, pr.CLOSE_REASON]


# ---------------------------------------------------------------- fuzz

def test_fuzz():
    streams = pr.fuzz_streams()
    assert len(streams) == 2000
    for masked in (False, True):
        check(streams, pr.R1, masked=masked, masked_call=masked, align=5)
