"""tests/proto_ref.py, the sequential model the protocol-check tests compare
with: pinned on its hand-typed known answers, and the seeded fuzz the GPU tests
use is accepted only if, by the model alone, it draws every verdict often enough
and leaves enough streams clean."""
from collections import Counter

import pytest

import proto_ref as pr


def test_values_match_the_public_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "kmws_gpu.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define KMWS_PROTO_([A-Z_]+)\s+(\d+)", txt)}
    assert got == {name: v for v, name in enumerate(pr.NAMES)}
    from kuma_amd import kmws
    for v, name in enumerate(pr.NAMES):
        assert getattr(kmws, "PROTO_" + name) == v


@pytest.mark.parametrize("case", pr.KNOWN, ids=[c[0] for c in pr.KNOWN])
def test_known_answers(case):
    _, rsv_allowed, frames, want, state = case
    assert len(want) == len(frames)
    got, after = pr.judge(frames, rsv_allowed)
    assert got == want
    assert after == state


def test_known_answers_cover_every_value_and_the_issues_list():
    seen = Counter(v for c in pr.KNOWN for v in c[3])
    assert set(seen) == set(range(11))
    names = {c[0] for c in pr.KNOWN}
    for code in (999, 1000, 1003, 1004, 1006, 1007, 1014, 1015, 2999, 3000, 4999, 5000):
        assert f"close_{code}" in names


@pytest.mark.parametrize("state,want", [(pr.IDLE, [0, 0, 4]), (pr.OPEN, [5, 10, 10]), (pr.CLOSED, [8, 8, 8]),
                                        (pr.FAILED, [10, 10, 10])])
def test_carried_state(state, want):
    frames = [pr.fr(pr.T, 0), pr.fr(pr.C, 1), pr.fr(pr.C, 1)]
    assert pr.judge(frames, 0, state)[0] == want


def test_splitting_a_stream_anywhere_changes_nothing():
    for s in pr.fuzz_streams(seed=5, n_streams=40):
        whole, end = pr.judge(s, pr.R1)
        for cut in range(len(s) + 1):
            a, mid = pr.judge(s[:cut], pr.R1)
            b, end2 = pr.judge(s[cut:], pr.R1, mid)
            assert a + b == whole and end2 == end


def test_fuzz_is_usable():
    streams = pr.fuzz_streams()
    assert len(streams) == 2000
    verdicts = [pr.judge(s, pr.R1)[0] for s in streams]
    n = sum(len(v) for v in verdicts)
    assert 30000 <= n <= 50000
    seen = Counter(v for vs in verdicts for v in vs)
    for v in range(11):
        assert seen[v] >= 50, (pr.NAMES[v], seen[v])
    clean = sum(1 for vs in verdicts if not any(vs))
    assert clean >= 0.30 * len(streams)
    assert pr.fuzz_streams() == streams  # seeded


def test_deliverable_stops_where_the_decoder_stops():
    s = [pr.fr(pr.T), pr.fr(pr.PING, 0), pr.fr(pr.T)]
    assert pr.deliverable(s) == s[:1]
    s = [pr.fr(pr.T), pr.close(999), pr.fr(pr.T)]
    assert pr.deliverable(s) == s[:2]
    s = [pr.fr(3), pr.fr(pr.PONG, payload=b"\0" * 126)]
    assert pr.deliverable(s) == s[:1]
    assert pr.wire_of([pr.fr(pr.T, payload=b"ab")]) == b"\x81\x02ab"
    assert pr.wire_of([pr.fr(pr.B, payload=b"\0" * 126)])[:4] == b"\x82\x7e\x00\x7e"
    assert pr.wire_of([pr.close(1000)], lambda i: b"\x01\x02\x03\x04") == b"\x88\x82\x01\x02\x03\x04\x02\xea"
