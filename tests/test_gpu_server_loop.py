"""A device-batch server's receive loop ("The receive
loop of a device batch") against the WSHandler drop-in and the references, on a
corpus whose reads end inside headers, keys, payloads and code points
(tests/server_loop.py; tests/test_server_loop_corpus.py proves the corpus
reaches what it must).  Every comparison is exact."""
import functools

import numpy as np
import pytest

import proto_ref as pr
import server_loop as sl
import utf8_ref as ref
from oracle import oracle as orc
from test_server_loop_corpus import N_CONN, references, the_corpus, the_model

pytestmark = pytest.mark.gpu
CAP = 128  # above every connection's frames in one round: the walk never stops at it


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    from kuma_amd import kmws
    if not torch.cuda.is_available() or kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")


@functools.lru_cache(maxsize=None)
def dropin():
    return sl.handler_loop(the_corpus())


@functools.lru_cache(maxsize=None)
def device(form, proto_first, cap=CAP):
    return sl.device_loop(the_corpus(), form, cap, proto_first)


@functools.lru_cache(maxsize=None)
def relay_references():
    """The UTF-8 reference of the reframe forms, per connection: (verdicts,
    state after, frames on which it is the plain reference too).  Under
    relay_opcodes = 0x0007 a frame with opcode 3-15 is not relayed, and
    kmws_unpack_reframe_utf8 judges the messages as they are emitted: such a
    frame is invisible (include/kmws_gpu.h: F[i] = 0x89, a FIN PING), where
    every other pass -- and the drop-in -- lets opcodes 3-7 open a message.  The
    two agree through a connection's first reserved data opcode; behind it
    (the protocol check has said OPCODE there, the connection is closing) each
    is held to its own contract."""
    out = []
    for d, _, _, uv, _ in references():
        v, st = ref.validate_stream([(f.b0 if f.b0 & 15 <= 2 else 0x89, f.payload) for f in d])
        same = next((j + 1 for j, f in enumerate(d) if 3 <= f.b0 & 15 <= 7), len(d))
        assert v[:same] == uv[:same]
        out.append((v, st, same))
    return out


def relayed(g, key):
    """The oracle's encoding of a relayed frame (empty for what relay_opcodes =
    0x0007 leaves to the host: control frames and reserved opcodes)."""
    if g.b0 & 15 > 2:
        return b""
    h = orc.Hdr(fin=g.b0 >> 7, rsv1=g.b0 >> 6 & 1, rsv2=g.b0 >> 5 & 1, rsv3=g.b0 >> 4 & 1, opcode=g.b0 & 15,
                mask=int(key is not None), maskey=key or b"\0\0\0\0", length=len(g.payload))
    return orc.encode_header(h) + (orc.mask_bytes(key, g.payload) if key else g.payload)


def test_the_drop_in_agrees_with_the_references():
    """handleData per read against proto_ref / utf8_ref and the host model of
    the loop: the frames of each read, both verdicts, the return code."""
    for i, (rounds, model) in enumerate(zip(dropin(), the_model())):
        d, pv, _, uv, _ = references()[i]
        assert len(rounds) == len(model), i
        k = 0
        for r, ((rc, got), (want, fail, tail)) in enumerate(zip(rounds, model)):
            assert [(g.b0, g.payload) for g in got] == want, (i, r)
            assert [g.proto for g in got] == pv[k:k + len(got)] and [g.utf8 for g in got] == uv[k:k + len(got)], (i, r)
            k += len(got)
            closed = bool(got) and got[-1].b0 & 15 == 8
            assert rc == (fail or (8 if closed else (1 if tail else 0))), (i, r, rc)
        assert k == len(d), i


@pytest.mark.parametrize("proto_first", [False, True])
@pytest.mark.parametrize("form", sl.FORMS)
def test_device_loop_equals_the_drop_in_read_by_read(form, proto_first):
    run, conns = device(form, proto_first), the_corpus().conns
    assert run.n_rounds == sl.R and run.max_live > 256 and run.max_frames > 1024
    assert run.n_classified == sum(1 for rounds in the_model() for _, fail, tail in rounds if tail) + \
        sum(1 for i, rounds in enumerate(the_model()) if rounds[-1][1] and i not in run.flat_fail)
    frames = 0
    for i, (dev, drop) in enumerate(zip(run.rounds, dropin())):
        d, pv, ps, uv, us = references()[i]
        same = len(d)
        if form.startswith("reframe"):
            uv, us, same = relay_references()[i]
        assert len(dev) == len(drop), f"connection {i}: {len(dev)} device rounds, {len(drop)} reads of the drop-in"
        k = fed = 0
        for r, ((got, fail, tail, relay, fed_dev), (rc, want)) in enumerate(zip(dev, drop)):
            at = f"connection {i} read {r}"
            # frames: count, header byte 0 and payload bytes of this read
            assert [(g.b0, g.payload) for g in got] == [(g.b0, g.payload) for g in want], at
            # return code: the failure code in the same read, 0 otherwise; a tail iff the drop-in wants more
            assert fail == (rc if rc in (5, 6, 7) else 0), f"{at}: device {fail}, handleData {rc}"
            assert bool(tail) == (rc == 1), at
            # verdicts: the drop-in's, and the two references'
            assert [g.proto for g in got] == [g.proto for g in want] == pv[k:k + len(got)], at
            assert [g.utf8 for g in got] == uv[k:k + len(got)], at
            assert [g.utf8 for g in got][:max(0, same - k)] == [g.utf8 for g in want][:max(0, same - k)], at
            assert all(g.err == 0 for g in got)
            if relay is not None:
                assert [b for b, _ in relay] == [relayed(g, key) for g, (_, key) in zip(got, relay)], at
            # tail: the masked bytes as they arrived, after the pass ran around them
            fed += len(conns[i].reads[r])
            assert fed_dev == fed and conns[i].wire[:fed].endswith(tail), at
            k += len(got)
        frames += k
        assert k == len(d), i
        # final carries (a connection that failed on a frame of the flat list was judged through that frame,
        # HEADER, and whatever the walk found behind it: the state is FAILED, the message state anything)
        if i in run.flat_fail:
            assert run.pcarry[i][0] == pr.FAILED and not run.pcarry[i][1:].any(), i
        else:
            assert run.pcarry[i][0] == ps and not run.pcarry[i][1:].any(), i
            assert (not run.ucarry[i].any()) == (not us.open), i
    assert frames == sum(len(r[0]) for r in references())
    print(f"{form} proto_first={proto_first}: {N_CONN} connections, {frames} frames, {run.n_rounds} rounds, "
          f"{run.n_classified} tails classified, at most {run.max_live} streams and {run.max_frames} frames a round")


def test_all_forms_give_identical_verdicts_and_carries():
    """Every form and both orders of the protocol check: the same frames and
    protocol verdicts everywhere; the same UTF-8 verdicts and carries among the
    unmask and gather forms and among the reframe forms, and across the two
    groups wherever their contracts coincide (relay_references)."""
    def verdicts(run, upto=None):
        return [[(g.b0, g.proto, g.utf8) for rnd in rounds for g in rnd[0]][:None if upto is None else upto[i]]
                for i, rounds in enumerate(run.rounds)]

    same = [s for _, _, s in relay_references()]
    base = device(sl.FORMS[0], False)
    flat = [v for c in verdicts(base) for v in c]
    seen_p, seen_u = sorted(set(p for _, p, _ in flat)), sorted(set(u for _, _, u in flat))
    for form in sl.FORMS:
        for proto_first in (False, True):
            run = device(form, proto_first)
            group = device("reframe" if form.startswith("reframe") else sl.FORMS[0], False)
            assert verdicts(run) == verdicts(group), form
            assert verdicts(run, same) == verdicts(base, same), form
            assert [[v[:2] for v in c] for c in verdicts(run)] == [[v[:2] for v in c] for c in verdicts(base)], form
            # (behind a refused frame the reframe, to which it is invisible, and the other passes, which judge it
            # as an empty frame, may leave different message states: those connections have failed)
            keep = [i for i in range(N_CONN) if i not in base.flat_fail]
            assert run.flat_fail == base.flat_fail and np.array_equal(run.pcarry, base.pcarry), form
            assert np.array_equal(run.ucarry[keep], group.ucarry[keep]), form
            # across the groups a kmws_utf8_carry is opaque but for "all zero = between messages"
            keep = [i for i in keep if not any(3 <= f.b0 & 15 <= 7 for f in references()[i][0])]
            assert np.array_equal(run.ucarry[keep].any(axis=1), base.ucarry[keep].any(axis=1)), form
            differ = [(i, bytes(run.ucarry[i]).hex(), bytes(base.ucarry[i]).hex()) for i in keep
                      if bytes(run.ucarry[i]) != bytes(base.ucarry[i])]
            if differ and not proto_first:
                print(f"{form}: {len(differ)} carries differ in their opaque bytes from the in-place form's:", differ[:8])
    print("proto verdicts seen:", [pr.NAMES[p] for p in seen_p], "utf8 verdicts seen:", seen_u)


def test_small_cap_lags_behind_the_reads_and_drains():
    """cap = 3: streams hit the cap, whole frames stay in the tail and the
    device loop falls behind the reads, so the comparison is per connection
    over the whole run; empty rounds follow the last read until the tails drain."""
    run = sl.device_loop(the_corpus(), "unmask", 3, False)
    assert run.n_rounds > sl.R
    for i, (dev, drop) in enumerate(zip(run.rounds, dropin())):
        d, pv, ps, uv, us = references()[i]
        got = [g for rnd in dev for g in rnd[0]]
        want = [g for _, gs in drop for g in gs]
        assert all(len(rnd[0]) <= 3 for rnd in dev), i
        assert [(g.b0, g.payload, g.proto, g.utf8) for g in got] == [(g.b0, g.payload, g.proto, g.utf8) for g in want], i
        assert [g.proto for g in got] == pv and [g.utf8 for g in got] == uv, i
        rc = drop[-1][0]
        assert all(not rnd[1] for rnd in dev[:-1]) and dev[-1][1] == (rc if rc in (5, 6, 7) else 0), i
        assert not dev[-1][2], f"connection {i}: a tail is left"
        wire = the_corpus().conns[i].wire
        assert all(wire[:rnd[4]].endswith(rnd[2]) for rnd in dev), f"connection {i}: a tail byte changed"
        if i not in run.flat_fail:
            assert run.pcarry[i][0] == ps and (not run.ucarry[i].any()) == (not us.open), i
    print(f"cap 3: {run.n_rounds} rounds for {sl.R} reads")


@pytest.mark.parametrize("form", ["gather", "unmask"])
def test_walking_on_behind_a_close_and_a_refused_frame(form):
    """Device only: the loop keeps a connection after its CLOSE and after an
    out_err frame.  The verdicts behind them -- AFTER_CLOSE; HEADER, then
    AFTER_FAIL -- reach later rounds through the proto carry and equal
    proto_ref.judge on the whole stream."""
    corp = sl.corpus_behind(77)
    run = sl.device_loop(corp, form, CAP, False, stop=False)
    seen, through_carry = set(), set()
    for i, (c, dev) in enumerate(zip(corp.conns, run.rounds)):
        got = [g for rnd in dev for g in rnd[0]]
        want, _ = pr.judge(c.frames, pr.R1)
        cut_short = bool(dev[-1][1])  # a refused header cut by a read fails at the tail: nothing behind it is walked
        assert len(got) == len(c.frames) or cut_short, i
        assert [g.proto for g in got] == want[:len(got)], i
        assert [g.b0 for g in got] == [f.b0 for f in c.frames[:len(got)]], i
        assert [bool(g.err) for g in got] == [bool(f.err) for f in c.frames[:len(got)]], i
        assert [g.payload for g in got if not g.err] == [f.payload for f in c.frames[:len(got)] if not f.err], i
        rounds_of = [r for r, rnd in enumerate(dev) for _ in rnd[0]]
        for k in range(1, len(got)):
            if rounds_of[k] != rounds_of[k - 1]:  # the first frame of a later round: the carry decided its verdict
                through_carry.add(got[k].proto)
        seen |= set(g.proto for g in got)
        if not cut_short:
            assert run.pcarry[i][0] == pr.judge(c.frames, pr.R1)[1], i
    assert {pr.AFTER_CLOSE, pr.HEADER, pr.AFTER_FAIL} <= seen
    assert {pr.AFTER_CLOSE, pr.AFTER_FAIL} <= through_carry, "no verdict came through a carry"


def test_a_tail_in_the_flat_list_is_parsed_with_the_neighbours_bytes():
    """The hazard the tail rule exists for, pinned.  Connection A's read ends
    after one header byte, `81`; connection B's begins `FE 00` (a complete
    empty frame) `05 80 ..`.  Passed in the flat list, A's tail is bounded by
    the next header offset for its payload but by wire_len for its header bytes
    (kmws_frame_parse.hpp unpack_one), so it is read as 81 FE 00 05: a masked
    126-class frame of length 5 -- INVALID_LENGTH (6), a connection failed for
    a header that has not arrived.  The loop's rule, one parse of the tail alone
    with wire_len = the stream's end, says NEED_MORE_DATA (1)."""
    import torch as T
    from kuma_amd import kmws
    wire = bytes([0x81]) + bytes([0xFE, 0x00]) + bytes([0x05, 0x80, 1, 2, 3, 4])
    d_wire = T.from_numpy(np.frombuffer(wire + bytes(23), dtype=np.uint8).copy()).cuda()
    desc = T.zeros((3, 2), dtype=T.int64, device="cuda")
    err = T.full((3,), 0xEE, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(kmws.lib().kmws_unpack_workspace_size())
    kmws.unpack_headers(d_wire, T.tensor([0, 1, 3], dtype=T.int64, device="cuda"), kmws.SERVER, desc, None, err, ws,
                        wire_len=len(wire))
    e = err.cpu().numpy().tolist()
    assert e == [6, 0, 0] and ws.status() == 2, \
        f"a cut tail `81` in the flat list in front of `FE 00 05` is reported as {e[0]} (6: bad length), not 1"
    kmws.unpack_headers(d_wire, T.tensor([0], dtype=T.int64, device="cuda"), kmws.SERVER, desc[:1], None, err[:1], ws,
                        wire_len=1)
    assert int(err[0]) == 1 and ws.status() == 2, "the tail alone, bounded by its stream's end, must wait for more"
