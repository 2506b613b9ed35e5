"""Pins tests/msg_ref.py, the model the GPU tests of kmws_msg_index compare
with, to known answers typed by hand: every case alone, all of them as the
streams of one batch, positions that are not dense, the verdicts of the last
member, and a stream cut into two batches."""
import pytest

import msg_ref as mr
import proto_ref as pr


@pytest.mark.parametrize("case", mr.KNOWN, ids=[k[0] for k in mr.KNOWN])
def test_known_answer(case):
    _, frames, carry_in, recs, msg_of, carry_after = case
    got = mr.walk([frames], mr.dense_pos([frames]), carries=[carry_in])
    assert got[0] == recs
    assert got[1] == msg_of
    assert got[2] == [0, len(recs)]
    assert got[3] == [carry_after]


def test_the_list_covers_what_the_rule_distinguishes():
    names = {k[0] for k in mr.KNOWN}
    assert {"one_frame", "three_fragments", "ping_with_payload_between", "empty_ping_between", "orphan_continue",
            "head_inside_open_message", "open_at_the_end", "continued_and_ended", "continued_not_ended",
            "only_control_frames_while_open", "empty_stream", "reserved_opcode_head"} <= names
    bits = {r["bits"] for k in mr.KNOWN for r in k[3]}
    assert {mr.BEGIN | mr.END | mr.CONTIG, mr.BEGIN | mr.END, mr.BEGIN | mr.CONTIG, mr.END | mr.CONTIG,
            mr.CONTIG} <= bits


def test_known_answers_as_one_batch():
    streams, carries, recs, msg_of, first_of, after = mr.known_batch()
    got = mr.walk(streams, mr.dense_pos(streams), carries=carries)
    assert got == (recs, msg_of, first_of, after)
    assert first_of[-1] == len(recs) == 16 and [r["stream"] for r in recs] == sorted(r["stream"] for r in recs)


def test_positions_decide_contig_and_off():
    frames = [pr.fr(pr.T, 0, payload=b"ab"), pr.fr(pr.PING, payload=b"??"), pr.fr(pr.C, 1, payload=b"cd")]
    # a gather that left the PING's payload elsewhere: the fragments are one run
    recs = mr.walk([frames], [100, 7, 102])[0]
    assert recs == [mr.rec(100, 4, 0, 0, 0, 2, 2, 1, mr.BEGIN | mr.END | mr.CONTIG)]
    recs = mr.walk([frames], [100, 7, 103])[0]
    assert recs == [mr.rec(100, 4, 0, 0, 0, 2, 2, 1, mr.BEGIN | mr.END)]
    # lengths past 2^32 and positions past 2^40
    big = 0xFFFFFFF0
    frames = [pr.fr(pr.B, 0), pr.fr(pr.C, 0), pr.fr(pr.C, 1)]
    p0 = 1 << 41
    recs, _, _, after = mr.walk([frames[:2]], [p0, p0 + big], lens=[big, big])
    assert recs == [mr.rec(p0, 2 * big, 0, 0, 0, 1, 2, 2, mr.BEGIN | mr.CONTIG)] and after == [mr.carry(2, 2 * big)]
    recs = mr.walk([frames[2:]], [p0 + 2 * big], lens=[big], carries=after)[0]
    assert recs == [mr.rec(p0 + 2 * big, big, 2 * big, 0, 0, 0, 1, 2, mr.END | mr.CONTIG)]


def test_verdicts_are_the_last_members():
    frames = [pr.fr(pr.T, 0), pr.fr(pr.PING), pr.fr(pr.C, 1), pr.fr(pr.PING)]
    recs = mr.walk([frames], [0, 0, 0, 0], utf8=[1, 0, 2, 0], proto=[0, 0, 0, 9])[0]
    assert [(r["utf8"], r["proto"]) for r in recs] == [(2, 0)]
    recs = mr.walk([frames[:2]], [0, 0], utf8=[1, 0], proto=[5, 10])[0]
    assert [(r["utf8"], r["proto"]) for r in recs] == [(1, 5)]


def test_two_batches_add_up():
    frames = [pr.fr(pr.T, payload=b"a"), pr.fr(pr.B, 0, payload=b"bc"), pr.fr(pr.PING, payload=b"p"),
              pr.fr(pr.C, 0, payload=b"def"), pr.fr(pr.C, 1, payload=b"g"), pr.fr(pr.C, 1, payload=b"orphan")]
    whole = mr.walk([frames], mr.dense_pos([frames]))
    assert [r["bytes"] for r in whole[0]] == [1, 6] and whole[3] == [mr.ZERO]
    for k in range(len(frames) + 1):
        a = mr.walk([frames[:k]], mr.dense_pos([frames[:k]]))
        b = mr.walk([frames[k:]], mr.dense_pos([frames[k:]]), carries=a[3])
        assert b[3] == whole[3]
        pieces = [r for r in a[0] + b[0] if r["b0"] == 2]
        assert sum(r["bytes"] for r in pieces) == 6
        assert [r["prior"] for r in pieces] == [0, pieces[0]["bytes"]][:len(pieces)]
        assert sum(bool(r["bits"] & mr.BEGIN) for r in pieces) == 1 and sum(bool(r["bits"] & mr.END) for r in pieces) == 1
