"""CPU proofs of tests/far_offset_cases.py, the host model behind
tests/test_gpu_far_offsets.py: every stride is odd, a batch of three periods
run through the oracle as ONE batch equals the period images repeated (so the
broadcast image is the oracle's answer for the whole device batch), and every
named lead puts on byte 2^31 / 2^32 exactly what its name says -- read back
from the descriptor arrays, not from the arithmetic that chose the lead."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import far_offset_cases as foc  # noqa: E402
import pack_edge_cases as pec  # noqa: E402
import utf8_ref as ref  # noqa: E402
from oracle import oracle as orc  # noqa: E402

PERIODS = ("chunk", "unit")
COPY_SPACES = foc.SPACES[1:]


@pytest.mark.parametrize("name", PERIODS)
def test_period_shape(name):
    p = foc.period(name)
    assert set(foc.PACKED_WIRE_LENS) <= set(p.lens.tolist())
    extra = set(p.lens.tolist()) - set(foc.PACKED_WIRE_LENS)
    assert all(L in pec.PHASE_LENS or L - 1 in pec.PHASE_LENS for L in extra)
    for space in COPY_SPACES:  # the form follows from the mean region alone
        S = p.geom(space)[0]
        assert pec.use_chunks(p.P, S) == (name == "chunk"), (space, S // p.P)
    assert p.b0[0] & 0x0F and p.b0[-1] & 0x80
    assert 0 in p.keys and any(0 in int(k).to_bytes(4, "little") and k for k in p.keys)
    assert 0 < p.enc_mask.sum() < p.P
    assert set(p.verdicts.tolist()) == {ref.OK, ref.NOT_TEXT}


@pytest.mark.parametrize("name", PERIODS)
def test_every_stride_is_odd_and_the_source_stride_is_its_own(name):
    p = foc.period(name)
    strides = {s: p.geom(s)[0] for s in foc.SPACES}
    assert all(S % 2 == 1 for S in strides.values()) and p.S_wire % 2 == 1, strides
    assert all(strides[s] != strides["src"] for s in COPY_SPACES), strides
    assert len({(k * strides["src"]) % 16 for k in range(16)}) == 16


def whole_source(L):
    fm, fp, fo = L.front_images()
    bad = lambda k: k == L.bad_row
    m = np.concatenate([fm] + [L.period_images(bad(k))[0] for k in range(L.reps)])
    u = np.concatenate([fp] + [L.period_images(bad(k))[1] for k in range(L.reps)])
    o = None if fo is None else np.concatenate([fo] + [L.period_images(bad(k))[2] for k in range(L.reps)])
    return m, u, o


def payloads_of(L):
    return [bytes(L.filler_payload())] * L.nf + L.p.payloads * L.reps


@pytest.mark.parametrize("name", PERIODS)
def test_tiling_in_place_images(name):
    """reps = 3 as one batch: the oracle's unmask of the whole masked source is
    the plain image repeated; the oracle's decoder finds the period's frames,
    keys and payloads three times (the header records and the gather image);
    the verdicts of the whole stream are the period's repeated, with no message
    left open."""
    p = foc.period(name)
    L = foc.Layout(p, "src", "payload_first_byte", reps=3)
    m, u, _ = whole_source(L)
    assert len(m) == L.src_bytes
    d = np.zeros(L.n, dtype=orc.DESC_DTYPE)
    d["off"], d["len"], d["key"] = L.pay_off, L.lens, L.keys
    got = m.copy()
    orc.unmask_batch(got, d)
    assert np.array_equal(got, u)
    for k in range(3):  # the decoder on each period's wire (the gap is not wire)
        a = L.front_src + k * p.S_src
        rets, fr = orc.decode_chunks(bytes(m[a:a + p.S_wire]), orc.SERVER, 0)
        assert rets == [0] and len(fr) == p.P
        assert [f.length for f in fr] == p.lens.tolist()
        assert [int.from_bytes(f.maskey, "little") for f in fr] == p.keys.tolist()
        assert [f.fin << 7 | f.opcode for f in fr] == p.b0.tolist() and all(f.mask for f in fr)
        assert b"".join(f.payload for f in fr) == bytes(p.dense)
        hdr = np.array([0] + np.cumsum([len(f.payload) + int(h) for f, h in zip(fr, p.hl)]).tolist())
        assert np.array_equal(hdr[:-1] + a, L.hdr_off[k * p.P:(k + 1) * p.P])
    out, st = ref.validate_stream(list(zip(L.b0.tolist(), payloads_of(L))))
    assert out == L.verdicts.tolist() and not st.open and not st.pending


@pytest.mark.parametrize("space", COPY_SPACES)
@pytest.mark.parametrize("name", PERIODS)
def test_tiling_copy_images(name, space):
    """reps = 3 as one batch through the oracle's encode_batch (for the gather:
    the plain concatenation) equals front image + period image x 3, and the
    offsets equal the cumsum."""
    p = foc.period(name)
    L = foc.Layout(p, space, "payload_first_byte", reps=3)
    m, u, o = whole_source(L)
    pays = payloads_of(L)
    if space == "gather":
        want, woff = np.frombuffer(b"".join(pays), np.uint8), np.cumsum([0] + [len(x) for x in pays])[:-1]
    elif space == "encode":  # from the plain source arena, at the absolute payload offsets
        fl = L.flags_out()
        keys = np.where(fl & foc.MASK, L.out_keys, 0)
        want, woff = orc.encode_batch(np.concatenate([u, np.zeros(16, np.uint8)]), L.pay_off, L.lens, fl, keys)
    else:                    # unmask each frame's slice of the masked source, encode with the outgoing keys
        d = np.zeros(L.n, dtype=orc.DESC_DTYPE)
        d["off"], d["len"], d["key"] = L.pay_off, L.lens, L.keys
        plain = m.copy()
        orc.unmask_batch(plain, d)
        fl = L.flags_out()
        keys = np.where(fl & foc.MASK, L.out_keys, 0)
        want, woff = orc.encode_batch(np.concatenate([plain, np.zeros(16, np.uint8)]), L.pay_off, L.lens, fl, keys)
    assert len(want) == L.out_bytes and np.array_equal(want, o)
    assert np.array_equal(np.asarray(woff, dtype=np.int64), L.out_off[:-1])
    out, st = ref.validate_stream(list(zip(L.b0.tolist(), pays)))
    assert out == L.verdicts.tolist() and not st.open


def holder(H, X):
    """The frame whose region starts last at or before X."""
    return int(np.searchsorted(H, X, side="right")) - 1


def check_lead(L):
    """What the descriptor arrays say lies on X."""
    p, X, lead = L.p, L.X, L.lead
    H, Pay, Len = L.aim_arrays()
    i = holder(H, X)
    j = (i - L.nf) % p.P
    cont = lambda b: 0x80 <= b <= 0xBF
    if lead == "payload_first_byte":
        assert Pay[i] == X and Len[i] == 70001 and j == p.J_BIG
    elif lead == "payload_last_byte_before":
        e = holder(Pay + Len, X)
        while Len[e] == 0:
            e -= 1
        assert Pay[e] + Len[e] == X and Len[e] == 70001
    elif lead == "header_straddles":
        assert H[i] < X < Pay[i] and j == p.J_BIG
        if Pay[i] - H[i] == 14:  # the key is bytes 10..13
            assert H[i] + 10 < X < H[i] + 14
    elif lead.startswith("key_phase_"):
        assert Pay[i] < X < Pay[i] + Len[i] and (X - Pay[i]) % 4 == int(lead[-1]) and Pay[i] % 16 != 0
    elif lead == "utf8_char_straddles":
        q = X - Pay[i]
        assert 1 <= q and q + 1 < Len[i] and L.b0[i] & 0x0F == 1
        assert 0xE0 <= L.payload_byte(i, q - 1) <= 0xEF
        assert cont(L.payload_byte(i, q)) and cont(L.payload_byte(i, q + 1))
        assert L.verdicts[i] == ref.OK
    elif lead == "utf8_fragment_edge":
        e = holder(Pay + Len, X)
        assert Pay[e] + Len[e] == X and Len[e] == 1000 and Len[e + 1] == 4096
        assert L.b0[e] == 0x01 and L.b0[e + 1] == 0x80  # text head without FIN, CONTINUE with FIN
        assert L.payload_byte(e, 999) == 0xE2 and [L.payload_byte(e + 1, k) for k in (0, 1)] == [0x82, 0xAC]
        assert L.verdicts[e] == ref.OK and L.verdicts[e + 1] == ref.OK
    else:
        a = X - foc.BAD_SHIFT[lead]
        i = holder(H, a)
        assert 0 <= a - Pay[i] < Len[i] and L.payload_byte(i, a - Pay[i]) == 0xFF
        row, j = divmod(i - L.nf, p.P)
        assert row == L.bad_row and j == p.J_TEXT
        v = L.verdicts
        bad = np.flatnonzero((v == ref.BAD) | (v == ref.AFTER_BAD))
        assert bad.tolist() == [i, i + 1, i + 2] and v[i] == ref.BAD  # that message's frames, no other period's
        others = np.delete(v[L.nf:].reshape(L.reps, p.P), row, axis=0)
        assert np.array_equal(others, np.tile(p.verdicts, (L.reps - 1, 1)))
        for k in (row - 1, row, row + 1):  # only that period holds the byte
            per = L.period_images(k == L.bad_row)[1]
            assert (int(per[p.pay_off[p.J_TEXT] + p.c1]) == 0xFF) == (k == row)
    if lead not in foc.BAD_SHIFT:
        assert L.bad_row is None and np.array_equal(L.verdicts[L.nf:L.nf + p.P], p.verdicts)


@pytest.mark.parametrize("X", (foc.X32, foc.X31), ids=("2^32", "2^31"))
@pytest.mark.parametrize("lead", foc.LEADS)
@pytest.mark.parametrize("space", foc.SPACES)
@pytest.mark.parametrize("name", PERIODS)
def test_lead_puts_on_the_boundary_what_it_names(name, space, lead, X):
    p = foc.period(name)
    L = foc.Layout(p, space, lead, X)
    check_lead(L)
    # the batch reaches past 2^32 + 2^27 in the source and, for a copy entry, in the output
    assert L.src_bytes >= foc.MIN_SPAN and L.pay_off[-1] > foc.X32 and np.all(np.diff(L.pay_off) >= 0)
    if L.copy:
        assert L.out_bytes >= foc.MIN_SPAN and L.out_off[-2] > foc.X32
        assert pec.use_chunks(L.n, L.out_bytes + 4096) == (name == "chunk")
        assert L.f < 10 << 20  # under the decoder's frame cap
