"""Pins tests/utf8_ref.py, the reference of the UTF-8 validator's tests, before
anything trusts it: over every string of length 1-4 over the boundary alphabet
(346,200 strings) whole-string validity equals bytes.decode("utf-8"), strict,
and the first bad fragment (one byte per fragment) equals a brute-force "no
completion decodes" search.  (codecs' incremental decoder is not a fail-fast
reference: CPython defers some verdicts, e.g. ED A0 split before 80.)"""
import itertools
import random

import utf8_ref as ref

ALPHABET = bytes.fromhex("007F808F909FA0BFC0C1C2DFE0E1ECEDEEEFF0F1F3F4F5FF")
# a viable prefix lacks at most three continuation bytes; 80, 90 and A0 between
# them satisfy every first-continuation range (E0: A0-BF, ED: 80-9F, F0: 90-BF,
# F4: 80-8F), and any of them every later one
_TAILS = [bytes(t) for k in range(4) for t in itertools.product((0x80, 0x90, 0xA0), repeat=k)]


def _decodes(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def _strings():
    for n in range(1, 5):
        for t in itertools.product(ALPHABET, repeat=n):
            yield bytes(t)


def test_whole_string_validity_is_bytes_decode():
    count = mismatches = 0
    for s in _strings():
        count += 1
        mismatches += ref.valid(s) != _decodes(s)
    assert count == 346200
    assert mismatches == 0


def test_first_bad_fragment_is_the_brute_force_search():
    viable = {b"": True}  # prefix -> some completion decodes

    def is_viable(p: bytes) -> bool:
        v = viable.get(p)
        if v is None:
            v = is_viable(p[:-1]) and any(_decodes(p + t) for t in _TAILS)
            viable[p] = v
        return v

    count = mismatches = 0
    for s in _strings():
        count += 1
        brute = next((k for k in range(len(s)) if not is_viable(s[:k + 1])), None)
        mismatches += ref.first_bad(s)[0] != brute
        # and through the message rules, one byte per fragment
        if len(s) == 3:
            got, _ = ref.validate_stream(ref.message([s[k:k + 1] for k in range(3)], fin=False))
            want = [ref.OK if brute is None or k < brute else (ref.BAD if k == brute else ref.AFTER_BAD)
                    for k in range(3)]
            mismatches += got != want
    assert count == 346200
    assert mismatches == 0


def test_message_rules():
    T, C, F = 1, 0, 0x80
    run = lambda frames: ref.validate_stream(frames)[0]
    euro = "€".encode()
    assert run([(T | F, euro)]) == [1]
    assert run([(2 | F, b"\xff")]) == [0] and run([(T | F | 0x40, b"\xff")]) == [0]
    assert run([(C | F, b"\xff")]) == [0]                      # CONTINUE with no open message
    assert run([(T, euro[:1]), (9 | F, b"\xff"), (C, euro[1:2]), (C | F, euro[2:])]) == [1, 0, 1, 1]
    assert run([(T, euro[:2]), (C | F, b"")]) == [1, 2]        # rule (b) on an empty FIN frame
    assert run([(T, euro), (C | F, b"")]) == [1, 1]
    assert run([(T, b"\xe0"), (C, b"\x80"), (C | F, b"a"), (T | F, b"a")]) == [1, 2, 3, 1]
    assert run([(T, b"\xc0"), (C | F, b"\x80")]) == [2, 3]
    assert run([(T, b"\xe2"), (T | F, b"ok")]) == [1, 1]      # a new head replaces the unfinished message
    out1, st = ref.validate_stream([(T, b"\xed")])
    assert out1 == [1] and ref.validate_stream([(C | F, b"\xa0\x80")], st)[0] == [2]


def test_generators_are_seeded_and_sized():
    a = ref.text(random.Random(3), 1000)
    assert a == ref.text(random.Random(3), 1000) and len(a) == 1000 and ref.valid(a)
    for w in ((1,), (3,), (1, 2, 3)):
        assert ref.valid(ref.text(random.Random(4), 999, w))
    parts = ref.fragment(random.Random(5), a, 7)
    assert b"".join(parts) == a
