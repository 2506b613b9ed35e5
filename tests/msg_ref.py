"""Sequential model of the message index (kmws_msg_index), written from the rule
as include/kmws_gpu.h states it: a plain walk over proto_ref's frame tuples, one
stream after the other; it never calls the library.  Known answers typed by
hand (tests/test_msg_ref.py pins the walk with them; the GPU tests run them on
the device).

A record is a dict with kmws_msg's fields; a carry is the 16 bytes of
kmws_msg_carry.
"""
import proto_ref as pr

NONE = 0xFFFFFFFF
BEGIN, END, CONTIG = 1, 2, 4
ZERO = bytes(16)
FIELDS = ("off", "bytes", "prior", "stream", "first", "last", "frames", "b0", "bits", "utf8", "proto")


def carry(b0, total):
    """The carry of an open message whose head byte 0 was b0, `total` bytes so far."""
    return bytes([0x80 | (b0 & 0x7F)]) + bytes(7) + total.to_bytes(8, "little")


def dense_pos(streams, lens=None):
    """Every frame's payload behind the one before, control frames included."""
    out, at, i = [], 0, 0
    for s in streams:
        for f in s:
            out.append(at)
            at += lens[i] if lens else len(f.payload)
            i += 1
    return out


def walk(streams, pos, lens=None, carries=None, utf8=None, proto=None):
    """-> (records, msg_of, stream_msg_first, carries after).  pos, lens (default:
    the payloads' lengths), utf8 and proto (default: zeros) are flat over all
    frames; carries: one per stream (default: none open)."""
    recs, msg_of, first_of, after = [], [], [0], []
    i = 0
    for s, frames in enumerate(streams):
        c = bytes(carries[s]) if carries is not None else ZERO
        is_open, b0, prior = bool(c[0] & 0x80), c[0] & 0x7F, int.from_bytes(c[8:], "little")
        cur = None  # the open message's record in this batch
        for f in frames:
            op, fin = f.b0 & 15, bool(f.b0 & 0x80)
            n = lens[i] if lens is not None else len(f.payload)
            member = False
            if op >= 8:
                pass
            elif op != 0:  # a head: replaces an unfinished message
                cur = dict(off=pos[i], bytes=0, prior=0, stream=s, first=i, last=i, frames=0, b0=f.b0 & 0x7F,
                           bits=BEGIN, utf8=0, proto=0)
                recs.append(cur)
                is_open, member = True, True
            elif is_open:
                if cur is None:  # open through the carry: its record starts here
                    cur = dict(off=pos[i], bytes=0, prior=prior, stream=s, first=i, last=i, frames=0, b0=b0, bits=0,
                               utf8=0, proto=0)
                    recs.append(cur)
                member = True
            if member:
                cur["bytes"] += n
                cur["frames"] += 1
                cur["last"] = i
                cur["_end"] = pos[i] + n
                cur["utf8"] = utf8[i] if utf8 is not None else 0
                cur["proto"] = proto[i] if proto is not None else 0
                msg_of.append(len(recs) - 1)
                if fin:
                    cur["bits"] |= END
                    is_open = False
            else:
                msg_of.append(NONE)
            i += 1
        if not is_open:
            after.append(ZERO)
        elif cur is None:
            after.append(c)  # no member in this batch: unchanged
        else:
            after.append(carry(cur["b0"], cur["prior"] + cur["bytes"]))
        first_of.append(len(recs))
    for r in recs:
        if r.pop("_end") - r["off"] == r["bytes"]:
            r["bits"] |= CONTIG
    return recs, msg_of, first_of, after


T, B, C, PING, PONG = pr.T, pr.B, pr.C, pr.PING, pr.PONG
fr = pr.fr


def rec(off, nbytes, prior, stream, first, last, frames, b0, bits, utf8=0, proto=0):
    return dict(off=off, bytes=nbytes, prior=prior, stream=stream, first=first, last=last, frames=frames, b0=b0,
                bits=bits, utf8=utf8, proto=proto)


# (name, frames of one stream, carry in, records with dense positions and stream 0 typed by hand (frame indices
#  from 0), msg_of typed by hand, carry after typed by hand)
KNOWN = [
    ("one_frame", [fr(T, payload=b"hello")], ZERO,
     [rec(0, 5, 0, 0, 0, 0, 1, 1, BEGIN | END | CONTIG)], [0], ZERO),
    ("three_fragments", [fr(B, 0, payload=b"ab"), fr(C, 0, payload=b"cde"), fr(C, 1, payload=b"f")], ZERO,
     [rec(0, 6, 0, 0, 0, 2, 3, 2, BEGIN | END | CONTIG)], [0, 0, 0], ZERO),
    ("ping_with_payload_between", [fr(T, 0, payload=b"ab"), fr(PING, payload=b"??"), fr(C, 1, payload=b"cd")], ZERO,
     [rec(0, 4, 0, 0, 0, 2, 2, 1, BEGIN | END)], [0, NONE, 0], ZERO),
    ("empty_ping_between", [fr(T, 0, payload=b"ab"), fr(PING), fr(C, 1, payload=b"cd")], ZERO,
     [rec(0, 4, 0, 0, 0, 2, 2, 1, BEGIN | END | CONTIG)], [0, NONE, 0], ZERO),
    ("orphan_continue", [fr(C, 1, payload=b"xx"), fr(T, payload=b"y"), fr(C, 0, payload=b"z")], ZERO,
     [rec(2, 1, 0, 0, 1, 1, 1, 1, BEGIN | END | CONTIG)], [NONE, 0, NONE], ZERO),
    ("head_inside_open_message", [fr(T, 0, payload=b"abc"), fr(B, 1, payload=b"de")], ZERO,
     [rec(0, 3, 0, 0, 0, 0, 1, 1, BEGIN | CONTIG), rec(3, 2, 0, 0, 1, 1, 1, 2, BEGIN | END | CONTIG)], [0, 1], ZERO),
    ("open_at_the_end", [fr(T, payload=b"a"), fr(B, 0, rsv=pr.R1, payload=b"bcd"), fr(C, 0, payload=b"ef")], ZERO,
     [rec(0, 1, 0, 0, 0, 0, 1, 1, BEGIN | END | CONTIG), rec(1, 5, 0, 0, 1, 2, 2, 0x42, BEGIN | CONTIG)], [0, 1, 1],
     carry(0x42, 5)),
    ("continued_and_ended", [fr(PING, payload=b"p"), fr(C, 0, payload=b"ab"), fr(C, 1, payload=b"c"), fr(T)],
     carry(0x02, 1000),
     [rec(1, 3, 1000, 0, 1, 2, 2, 2, END | CONTIG), rec(4, 0, 0, 0, 3, 3, 1, 1, BEGIN | END | CONTIG)],
     [NONE, 0, 0, 1], ZERO),
    ("continued_not_ended", [fr(C, 0, payload=b"abcd"), fr(PONG), fr(C, 0)], carry(0x41, (1 << 32) + 5),
     [rec(0, 4, (1 << 32) + 5, 0, 0, 2, 2, 0x41, CONTIG)], [0, NONE, 0], carry(0x41, (1 << 32) + 9)),
    ("only_control_frames_while_open", [fr(PING, payload=b"abc"), fr(PONG), pr.close(1000)], carry(0x01, 77),
     [], [NONE, NONE, NONE], carry(0x01, 77)),
    ("empty_stream_open", [], carry(0x02, 3), [], [], carry(0x02, 3)),
    ("empty_stream", [], ZERO, [], [], ZERO),
    ("reserved_opcode_head", [fr(5, 0, payload=b"ab"), fr(C, 1, payload=b"c"), fr(7, payload=b"d")], ZERO,
     [rec(0, 3, 0, 0, 0, 1, 2, 5, BEGIN | END | CONTIG), rec(3, 1, 0, 0, 2, 2, 1, 7, BEGIN | END | CONTIG)],
     [0, 0, 1], ZERO),
    ("head_replaces_carried_message", [fr(T, payload=b"abc")], carry(0x02, 9),
     [rec(0, 3, 0, 0, 0, 0, 1, 1, BEGIN | END | CONTIG)], [0], ZERO),
    ("header_error_frame_by_its_flags", [fr(T, 0, payload=b"ab"), fr(C, 1, err=6), fr(C, 1, payload=b"x")], ZERO,
     [rec(0, 2, 0, 0, 0, 1, 2, 1, BEGIN | END | CONTIG)], [0, 0, NONE], ZERO),
]


def known_batch():
    """The known answers as the streams of one batch: (streams, carries, records,
    msg_of, stream_msg_first, carries after), positions dense over the batch."""
    streams = [k[1] for k in KNOWN]
    carries = [k[2] for k in KNOWN]
    recs, msg_of, first_of, after = [], [], [0], []
    frame0 = at = 0
    for s, (_, frames, _, rs, mo, ca) in enumerate(KNOWN):
        for r in rs:
            recs.append(dict(r, off=r["off"] + at, stream=s, first=r["first"] + frame0, last=r["last"] + frame0))
        msg_of += [NONE if m == NONE else m + first_of[-1] for m in mo]
        first_of.append(len(recs))
        after.append(ca)
        frame0 += len(frames)
        at += sum(len(f.payload) for f in frames)
    return streams, carries, recs, msg_of, first_of, after
