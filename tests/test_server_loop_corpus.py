"""The conditions that keep tests/test_gpu_server_loop.py informative, checked
without a GPU on the references alone (proto_ref.judge, utf8_ref.validate_stream,
proto_ref.deliverable, the host walk kmws.find_headers): the corpus of
tests/server_loop.py reaches every verdict, every kind of read cut and every
wire-level error, and the loop's bookkeeping -- compaction rule, tail rule --
applied read by read on the host delivers exactly proto_ref.deliverable's
frames.  If a condition fails, the corpus changes, not the condition."""
import functools

import proto_ref as pr
import proto_util as pu
import server_loop as sl
import utf8_ref as ref

SEED, N_CONN = 20261021, 400


@functools.lru_cache(maxsize=None)
def the_corpus():
    return sl.corpus(SEED, N_CONN)


@functools.lru_cache(maxsize=None)
def the_model():
    from kuma_amd import kmws
    return sl.model_loop(the_corpus(), kmws.find_headers)


@functools.lru_cache(maxsize=None)
def references():
    """Per connection: (deliverable frames, proto verdicts, state after, UTF-8 verdicts, state after)."""
    out = []
    for c in the_corpus().conns:
        d = pr.deliverable(c.frames)
        pv, ps = pr.judge(d, pr.R1)
        uv, us = ref.validate_stream([(f.b0, f.payload) for f in d])
        out.append((d, pv, ps, uv, us))
    return out


def cuts_of(c):
    """[(read index r, byte position)]: read r ends at that position."""
    pos, out = 0, []
    for r, rd in enumerate(c.reads[:-1]):
        pos += len(rd)
        out.append((r, pos))
    return out


def cut_kinds(i):
    """The kinds of read cut (sl.CUT_KINDS) connection i really goes through:
    only reads the loops still feed count, and only frames in front of its stop."""
    corp, model = the_corpus(), the_model()
    c, rounds = corp.conns[i], model[i]
    d, _, _, uv, _ = references()[i]
    kinds = set()
    for r, q in cuts_of(c):
        if r >= len(rounds):
            break
        for j, (o, hl, pl) in enumerate(c.layout[:len(d)]):
            if q == o + 1:
                kinds.add("hdr0")
            if hl in (8, 14) and o + 2 < q < o + hl - 4:
                kinds.add("ext2" if hl == 8 else "ext8")
            if o + hl - 4 < q < o + hl:
                kinds.add("key")
            if o + hl < q < o + hl + pl:
                kinds.add("payload")
                if uv[j] == ref.OK and c.frames[j].payload[q - o - hl] & 0xC0 == 0x80:
                    kinds.add("codepoint")
            if q == o and j >= 1:
                kinds.add("boundary")
        closed = d and d[-1].b0 & 15 == 8  # then the next frame lies behind the CLOSE: never reached
        if not closed and len(d) < len(c.frames) and c.raw[len(d)] in ("len126", "len127"):
            o, ext = c.layout[len(d)][0], 2 if c.raw[len(d)] == "len126" else 8
            if c.raw[len(d)] == "len127" and o + 2 < q < o + 10:
                kinds.add("ext8")
            later = any(len(model[k]) > r and corp.conns[k].reads[r] for k in range(i + 1, len(corp.conns)))
            if o + 2 <= q <= o + 2 + ext and later:
                kinds.add("badlen_tail")
    for r, (got, fail, tail) in enumerate(rounds):
        if not c.reads[r]:
            kinds.add("empty")
        elif not got and not fail:
            kinds.add("noframe")
    return kinds


def test_every_reachable_proto_value_occurs():
    """HEADER and CONTROL need a frame the decoder refuses and AFTER_CLOSE one
    behind a CLOSE: neither is delivered (the variant that keeps walking covers
    HEADER and AFTER_CLOSE; the parse turns a CONTROL frame into HEADER)."""
    seen = set(v for _, pv, _, _, _ in references() for v in pv)
    assert seen == {pr.OK, pr.RSV, pr.OPCODE, pr.CONTINUATION, pr.INTERLEAVED, pr.CLOSE_PAYLOAD, pr.CLOSE_REASON,
                    pr.AFTER_FAIL}, sorted(pr.NAMES[v] for v in seen)
    assert {ps for _, _, ps, _, _ in references()} == {pr.IDLE, pr.OPEN, pr.CLOSED, pr.FAILED}


def test_all_four_utf8_verdicts_occur():
    seen = set(v for _, _, _, uv, _ in references() for v in uv)
    assert seen == {ref.NOT_TEXT, ref.OK, ref.BAD, ref.AFTER_BAD}
    assert {us.open for _, _, _, _, us in references()} == {False, True}


def test_close_endings_good_bad_code_bad_reason():
    ends = set(pv[-1] for d, pv, _, _, _ in references() if d and d[-1].b0 & 15 == 8 and len(d[-1].payload) >= 2)
    assert {pr.OK, pr.CLOSE_PAYLOAD, pr.CLOSE_REASON} <= ends


def test_every_cut_kind_on_at_least_three_connections():
    count = {k: 0 for k in sl.CUT_KINDS}
    for i in range(N_CONN):
        for k in cut_kinds(i):
            count[k] += 1
    assert all(v >= 3 for v in count.values()), count


def test_messages_and_code_points_span_reads():
    spans = 0
    for i, c in enumerate(the_corpus().conns):
        d = references()[i][0]
        ends = [q for _, q in cuts_of(c)]
        read_of = lambda p: sum(1 for q in ends if q <= p)  # noqa: E731
        head = None
        for j, f in enumerate(d):
            if f.b0 & 15 in (1, 2):
                head = j
            if f.b0 & 15 < 8 and f.b0 & 0x80 and head is not None:
                o, hl, pl = c.layout[j]
                if read_of(o + hl + pl - 1) - read_of(c.layout[head][0]) >= 2:
                    spans += 1
                head = None
    assert spans >= 3, "no message spans three reads"
    assert sum("codepoint" in cut_kinds(i) for i in range(N_CONN)) >= 3


def test_at_least_ten_empty_stream_rounds():
    n = sum(1 for rounds in the_model() for got, fail, tail in rounds if not got and not fail)
    assert n >= 10, n


def test_every_wire_level_error_kind_is_reached():
    seen = set()
    for i, c in enumerate(the_corpus().conns):
        d = references()[i][0]
        if c.raw and c.raw[-1] and len(d) == len(c.frames) - 1 and not (d and d[-1].b0 & 15 == 8):
            assert the_model()[i][-1][1] == sl.ERR_KINDS[c.raw[-1]] == c.frames[-1].err
            seen.add(c.raw[-1])
    assert seen == set(sl.ERR_KINDS)


def test_lengths_cover_the_header_class_edges():
    lens = set(len(f.payload) for d, _, _, _, _ in references() for f in d)
    assert {0, 125, 126, 65535, 65536} <= lens
    big = [i for i, (d, _, _, _, _) in enumerate(references()) if any(len(f.payload) > 300 for f in d)]
    assert 3 <= len(big) <= 10 and all(len(f.payload) <= 300 or len(f.payload) in sl.BIG
                                       for c in the_corpus().conns for f in c.frames)


def test_one_round_is_wide_deep_and_holds_a_64k_frame():
    model = the_model()
    ok = []
    for r in range(sl.R):
        live = sum(1 for rounds in model if len(rounds) > r)
        frames = sum(len(rounds[r][0]) for rounds in model if len(rounds) > r)
        big = any(len(p) == 65536 for rounds in model if len(rounds) > r for _, p in rounds[r][0])
        ok.append((live, frames, big))
    assert any(live > 256 and frames > pu.block_frames() and big for live, frames, big in ok), ok


def test_host_walk_read_by_read_delivers_the_deliverable_frames():
    """The loop's bookkeeping without a GPU: compaction rule, tail rule and the
    per-tail classification give proto_ref.deliverable's frames, the stop's
    WSError in the read that completes the refused header, and no tail left."""
    for i, (c, rounds) in enumerate(zip(the_corpus().conns, the_model())):
        d = references()[i][0]
        got = [x for g, _, _ in rounds for x in g]
        assert got == [(f.b0, f.payload) for f in d], i
        assert all(not fail for _, fail, _ in rounds[:-1]), i
        fail, tail = rounds[-1][1], rounds[-1][2]
        if d and d[-1].b0 & 15 == 8:
            assert not fail and len(rounds) <= sl.R, i
        elif len(d) < len(c.frames):
            assert fail == (c.frames[len(d)].err or 7), i  # a synthetic stop is a control frame the parse refuses
        else:
            assert not fail and not tail and len(rounds) == sl.R, i
        fed = 0
        for r, (_, _, t) in enumerate(rounds):
            fed += len(c.reads[r])
            assert c.wire[:fed].endswith(t), i
