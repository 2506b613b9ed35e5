"""CPU checks of tests/pack_edge_cases.py: the structural constants the cases
are aimed at still have the values in the kernel source, every named case has
the property its name claims (by the module's geometry model), and the oracle
encodes every case.  The device runs are in tests/test_gpu_pack_edges.py."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pack_edge_cases as pec  # noqa: E402
from oracle import oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kuma_amd", "csrc")


def _constexpr_defs():
    text = ""
    for name in ("kmws_common.hpp", "kmws_workspace.hpp", "kmws_pack.hip"):
        with open(os.path.join(CSRC, name)) as f:
            text += f.read()
    text = re.sub(r"//[^\n]*", "", text)
    return dict(re.findall(r"constexpr\s+[\w\s]+?\b(k[A-Z]\w*)\s*=\s*([^;]+);", text))


def _value(name, defs):
    """A constexpr integer of the source: literals, casts, other constants, * + - / << ( )."""
    expr = re.sub(r"\((?:int|uint32_t|uint64_t)\)", "", defs[name])
    expr = re.sub(r"\b(\d+)(?:ull|ul|ll|u|l)\b", r"\1", expr, flags=re.I)
    expr = re.sub(r"\bk[A-Z]\w*", lambda m: str(_value(m.group(0), defs)), expr)
    assert re.fullmatch(r"[\d\s*+\-/()<]+", expr), (name, expr)
    return eval(expr.replace("/", "//"))  # integers only (checked above)


def test_constants_match_the_kernel_source():
    """A retune of kmws_pack.hip moves the cases off their edges: fail here first."""
    defs = _constexpr_defs()
    got = {name: _value(name, defs) for name in pec.CONSTANTS}
    assert got == pec.CONSTANTS
    # the form rule the device tests select the form with
    with open(os.path.join(CSRC, "kmws_workspace.hpp")) as f:
        assert re.search(r"copy_uses_chunks\(uint32_t n, uint64_t cap\)\s*\{\s*return n && cap / n < kChunkFormBelow;",
                         f.read())


def _variants():
    return [(name, h) for name, c in pec.CASES.items() for h in c.variants()]


def test_the_issue_s_cases_are_all_there():
    want = {"chunk": 12, "empty": 4, "unit": 15}
    have = {g: sum(c.group == g for c in pec.CASES.values()) for g in want}
    assert have == want
    for name, c in pec.CASES.items():
        if c.group == "empty":
            assert c.variants() == [False], name  # encode regions are never empty


@pytest.mark.parametrize("name,headers", _variants())
def test_case_has_the_property_its_name_claims(name, headers):
    case = pec.CASES[name]
    src, offs, lens, flags, keys = case.build(headers)
    g = pec.Geometry(offs, lens, flags, headers)
    case.check(g)
    # the builder's own contract: payloads inside the arena, disjoint, in order
    end = offs.astype(np.int64) + lens
    assert np.all(end[:-1] <= offs.astype(np.int64)[1:]) and end[-1] + 16 <= len(src)
    assert g.n <= 4097 and np.all(lens >= 0)
    if g.n > 6:
        assert np.any(keys == 0) and np.any(keys != 0)
    # both forms are reachable through dst_cap alone
    assert pec.use_chunks(g.n, g.total + 5000)
    assert not pec.use_chunks(g.n, max(g.total, pec.kChunkFormBelow * g.n) + 777)


@pytest.mark.parametrize("name,headers", _variants())
def test_oracle_encodes_every_case(name, headers):
    """Encode variant: its own frames.  Gather variant: the masked wire the
    fused unpack-gather reads (payload lengths = the case's regions)."""
    src, offs, lens, flags, keys = pec.CASES[name].build(headers)
    wire, wire_off = orc.encode_batch(src, offs, lens, flags, keys)
    g = pec.Geometry(offs, lens, flags, True)
    assert len(wire) == g.total and np.array_equal(wire_off.astype(np.int64), g.r0)
    masked = (flags >> 8) & 1 == 1
    assert headers or masked.all()
    for f in {0, g.n // 2, g.n - 1}:  # the payload bytes are where the model says
        key = np.frombuffer(int(keys[f] if masked[f] else 0).to_bytes(4, "little"), np.uint8)
        pay = src[int(offs[f]):int(offs[f]) + int(lens[f])] ^ np.resize(key, int(lens[f]))
        assert np.array_equal(wire[int(g.p0[f]):int(g.r1[f])], pay), f


@pytest.mark.parametrize("n", pec.COUNT_EDGES)
def test_frame_count_batches(n):
    for headers in (True, False):
        src, offs, lens, flags, keys = pec.frame_count_batch(n, headers)
        assert len(lens) == n and set(lens) <= set(pec.COUNT_LENS)
        g = pec.Geometry(offs, lens, flags, headers)
        # every whole row and tile holds every length, so no two rows or tiles share a prefix pattern
        for a in range(0, n - pec.kBlock + 1, pec.kBlock):
            assert set(lens[a:a + pec.kBlock]) == set(pec.COUNT_LENS)
        assert pec.use_chunks(n, g.total + 5000) and pec.kChunkFormBelow * n + 777 <= 70 << 20
        if headers:
            assert len(set(flags)) == 2  # masked and unmasked
            orc.encode_batch(src, offs, lens, flags, keys)


@pytest.mark.parametrize("headers,mixed", [(True, False), (True, True), (False, False)])
def test_every_phase_pair_occurs_on_an_interior_word(headers, mixed):
    """Over the 16 batches: every (source phase, output phase) pair with every
    length class; the pair's long frames have interior words in both forms."""
    seen, interior_chunk, interior_unit = set(), set(), set()
    for po in range(16):
        src, offs, lens, flags, keys = pec.phase_batch(po, headers, mixed)
        g = pec.Geometry(offs, lens, flags, headers)
        w = g.frame_words()
        test = np.arange(g.n) % 2 == 1  # pad, frame, pad, frame ...
        assert np.all(g.p0[test] % 16 == po) and np.all(lens[~test] < 16)
        for f in np.nonzero(test)[0]:
            pair = (int(offs[f]) % 16, int(g.p0[f]) % 16)
            assert (pair[0] - pair[1]) % 16 == g.delta[f]
            seen.add(pair + (int(lens[f]),))
            if (g.p0[f] + 15) // 16 * 16 + 16 <= g.r1[f]:
                interior_chunk.add(pair)
            if w["ihi"][f] > w["ilo"][f]:
                interior_unit.add(pair)
        assert np.any(keys[test] == 0) and np.any(keys[test] != 0)
        if headers:
            assert len(set(flags[test])) == (2 if mixed else 1)
            orc.encode_batch(src, offs, lens, flags, keys)
        assert g.n <= 4097 and pec.use_chunks(g.n, g.total + 5000)
    pairs = {(a, b) for a in range(16) for b in range(16)}
    assert seen == {p + (L,) for p in pairs for L in pec.PHASE_LENS}
    assert interior_chunk == pairs and interior_unit == pairs
